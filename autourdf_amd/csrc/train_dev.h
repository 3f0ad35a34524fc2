// train_dev.h -- what the train plan's translation units share (train_engine.hip: the plan, the epoch, graph capture and the
// public entries; train_setup.hip: staging, the once-per-train sorts, state in / out; train_forward.hip: k_l2 and k_head;
// train_nn.hip: the nearest-neighbour launch; train_backward.hip: k_gradc and k_bd): the shape and workspace structs every kernel
// takes, the few device helpers more than one unit needs, the limits make_dims shares with the kernels they bound, and the units'
// host interface.  This build has no relocatable device code: a kernel is launched by the unit that defines it, so every unit
// carries its own launchers and train_engine.hip launches no train kernel itself.
#pragma once
#include <type_traits>
#include "creg_common.h"
#include "creg_dev.h"

namespace creg {

struct Dims {
    int rot, K, KP, IN, H, HA, HB, H2, OA, OB, NP, NT, epochs;      // KP: K rounded up to the k_bd D role's contraction chunk (rows K..KP-1 of x1 / h2 / g_h2 / g_out stay 0)
    float slope;
    // flat parameter offsets
    int oW1, ob1, oW2, ob2, oW3A, ob3A, oW3B, ob3B, NPAR;
    int nbx, nby;  // NN blocks per direction (= loss partial counts)
    int nyb;       // 64-point blocks of the sorted target frame (0: exhaustive search only)
    int npb;       // upper bound of the blocks of the predicted cloud, clusters padded (0: that direction exhaustive)
    int ppl;       // points per lane and block visit: blocks hold 64 * ppl points
    int nbt, nbp;  // boxes per lane of the search over the target frame / the predicted cloud (their box tables hold 64 nbt / 64 nbp)
    int rows;      // the search takes sixteen queries per wave in slot order (nn_l1_rows, round 5): loss partials per 16-slot group
};

constexpr int PS_MAXB = 512;                   // most blocks of the predicted cloud (clusters padded): eight boxes per lane in the search
constexpr int YS_CHUNK = 16384;                // most slots one workgroup sorts in LDS (k_sort_y cuts longer frames into chunks of this size: see there)

struct Hyper {      // uploaded per run
    float lr, factor;
    int patience, stop;
};

struct TrainState {
    double lr, sched_best;
    int sched_bad, count, stopped, step;
    float min_loss;
    int epochs_run, best_epoch;
    float step_size, bc2_sqrt;   // Adam scalars for the update of the epoch that produced this state
    float last_loss;
    float next_bc2s;             // bias corrections of step `step + 1` (k_prep's tables), fetched by the epoch that produced
    double next_bc1;             //   this state: the next epoch reads them WITH the state instead of in a round trip after it
};

struct Ws {         // device pointers into the caller's workspace
    float *P, *P1, *AM, *AV;     // parameters double-buffered by optimizer-step parity: epoch e reads P[e & 1] (P / P1) and writes the
                                 //   other one, so no kernel of an epoch can see a row another workgroup has already updated
    float *pose_in, *enc, *x1[2], *h2[2], *head_save, *m2, *gm2;      // x1 / h2: double-buffered by epoch parity
    float4 *pts4, *y4, *pred4, *ys4, *psl4, *ps4;
    float *ybox, *pbox;
    int* sb;
    int* sgn_x;
    int4* cnt4;
    float *lossp_x, *lossp_y;
    float *g_out, *g_h2;
    TrainState* state;
    double* bc1;        // [epochs + 1] Adam bias corrections by step, filled once per train by k_prep:
    float* bc2s;        //   1 - 0.9^t and sqrt(1 - 0.999^t) (two double pow() off the per-epoch critical path)
    float *best_m, *best_pred, *loss_hist, *lr_hist, *result;
    int* off;
    Hyper* hyper;
    unsigned long long* ysum;   // [4] per chunk of the target frame: fingerprint of the points its k-d leaves were built from (k_sort_y)
};

// Problem b of a batch lives in its own copy of the workspace layout, `bytes` = b * stride further on:
// every member of Ws is a pointer, so shifting the struct is shifting each of them.
static_assert(sizeof(Ws) % sizeof(char*) == 0, "Ws must hold pointers only");
__host__ __device__ __forceinline__ Ws ws_shift(Ws W, size_t bytes) {
    char** p = reinterpret_cast<char**>(&W);
#pragma unroll
    for (size_t i = 0; i < sizeof(Ws) / sizeof(char*); ++i) p[i] += bytes;
    return W;
}

// pose representations of train() (mlp_reg.py:64-90; creg_train_shape.rot)
constexpr int ROT_Q = 0, ROT_DQ = 1, ROT_6D = 2, ROT_RPY = 3;
constexpr int POSE_IN = 12;            // floats per pose row of the model input (q: 7, dq: 8, 6d: 9, rpy: 6)
typedef float f32x4 __attribute__((ext_vector_type(4)));       // an MFMA 16x16x4 accumulator (k_l2, k_bd)
typedef float nn_f2 __attribute__((ext_vector_type(2)));       // (nn_l1.h's pair type, the same declaration: k_bd stores pairs)
__device__ __forceinline__ float act_f(float v, float slope) { return v > 0.f ? v : v * slope; }
__device__ __forceinline__ float act_grad(float post, float slope) { return post > 0.f ? 1.f : slope; }

__device__ __forceinline__ int seg_of(const int* __restrict__ off, int k, int n) {
    int lo = 0, hi = k;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= n) lo = mid; else hi = mid; }
    return lo;
}

// ---- measurement build -DCREG_BD_STAMPS (tests/measure/bd_stamps.py): the phase stamps of k_bd's two roles.  g_bd_st, what the
//      stamps are summed into, is train_backward.hip's; the default build drops the statements before it parses them.
#ifdef CREG_BD_STAMPS
#define BD_T0 unsigned long long bd_t[8]; int bd_n = 0; if (threadIdx.x == 0) bd_t[bd_n++] = bd_entry;
#define BD_T  if (threadIdx.x == 0) bd_t[bd_n++] = wall_clock64();
#define BD_TEND(role, epoch) do { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); if (threadIdx.x == 0) { bd_t[bd_n++] = wall_clock64(); \
    if (g_bd_st.armed) { const int sl_ = (epoch) & 255; atomicMin(&g_bd_st.first[sl_], bd_t[0]); \
        atomicMin(role ? &g_bd_st.startD[sl_] : &g_bd_st.startB[sl_], bd_t[0]); atomicMax(role ? &g_bd_st.endD[sl_] : &g_bd_st.endB[sl_], bd_t[bd_n - 1]); \
        for (int k_ = 1; k_ < bd_n; ++k_) atomicAdd(&g_bd_st.phase[role][k_ - 1], bd_t[k_] - bd_t[k_ - 1]); atomicAdd(&g_bd_st.blocks[role], 1ull); } } } while (0)
#else
#define BD_T0
#define BD_T
#define BD_TEND(role, epoch)
#endif

// ---- host side
constexpr int BATCH_MAX = 64;                      // problems of a plan (k_prep's argument tables)
// The problems one launch covers: the first one's workspace and how many follow it, `bstride` bytes apart (the launch's grid.z).
struct Slice { Ws W; int nz; };

// A run-time value as a template argument: f(integral_constant<V>) for the listed V that equals v, the last one if none does.
template <int V, int... Vs, typename F>
static void by_value(int v, F f) {
    if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V>{});
    else if (v == V) f(std::integral_constant<int, V>{});
    else by_value<Vs...>(v, f);
}
// the kernel instance of a hidden width: NC = H / 64, H in {64, 128, 256, 512}
template <typename F>
static void by_nc(int H, F f) { by_value<1, 2, 4, 8>(H / 64, f); }

// ---- the units as train_engine.hip sees them: one launcher per launch.  Arguments are checked by the public entries; a launcher
//      only enqueues on `s` (the caller looks at hipGetLastError).  The *_raise_lds functions lift the dynamic-LDS limit of their
//      unit's kernels on the current device.
// train_setup.hip
struct ParamMap { int off, count; };
int param_map(const Dims& D, ParamMap* pm);        // where each of the caller's parameter tensors lives in the flat buffer; returns their count (10, 'dq': 6)
constexpr int COPY_MAX = 150;                      // ranges per k_copy_table launch (3.1 KB of kernel arguments)
struct CopyTable { const unsigned* src[COPY_MAX]; unsigned* dst[COPY_MAX]; int n[COPY_MAX]; int count = 0; };
void copy_table_add(CopyTable& T, const void* src, void* dst, size_t bytes, hipStream_t s);      // launches when full
void copy_table_launch(CopyTable& T, hipStream_t s);
int setup_raise_lds(const Dims& D);
int stage_inputs(const Dims& D, const Slice& S, size_t bstride, const creg_train_args* args, hipStream_t s);
void launch_sorts(const Dims& D, const Slice& S, size_t bstride, hipStream_t s, bool keep_target_blocks);
void launch_params_home(const Dims& D, const Slice& S, size_t bstride, int sidx, int step0, hipStream_t s);
void launch_set_state(const Dims& D, const Ws& W, const creg_train_state& from, hipStream_t s);
void launch_get_state(const Ws& W, int sidx, double* out, hipStream_t s);
// train_forward.hip
void launch_l2(const Dims& D, const Slice& S, size_t bstride, int par, hipStream_t s);
void launch_head(const Dims& D, const Slice& S, size_t bstride, int par, hipStream_t s);
// train_nn.hip
void launch_nn(const Dims& D, const Slice& S, size_t bstride, int par, hipStream_t s);
// train_backward.hip
bool backward_fits(const Dims& D);                 // the shape limits of k_gradc and k_bd (make_dims)
int bd_raise_lds(const Dims& D);
void launch_gradc(const Dims& D, const Slice& S, size_t bstride, int epoch, hipStream_t s);
void launch_bd(const Dims& D, const Slice& S, size_t bstride, int epoch, hipStream_t s);
int bd_stamps_arm(bool on);                        // -DCREG_BD_STAMPS: clear and arm / disarm the stamps; nothing in the default build

}  // namespace creg
