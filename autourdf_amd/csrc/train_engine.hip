// train_engine.hip -- A1: the whole `train` loop of the reference (PointCloud/mlp_reg.py:17-152)
// as a device-resident plan.  One epoch = FIVE small launches (enqueue_epoch), no host round trip; every parameter
// row is read once per epoch, by the role that updates it:
//
//   k_head    output layer(s) + residual + pose assembly + calculate_pc (mlp_reg.py:62-94,155-170),
//             one workgroup per pose row / cluster
//   NN        L1 nearest neighbour both ways (chamfer_distance, mlp_reg.py:96): k_nn_rows, k_nn_plan or k_nn_l1 by
//             problem size (launch_nn); its epilogue emits the loss partials and the sign scatter of the y->x term
//             (integer atomics: exact)
//   k_gradc   loss, best tracking (mlp_reg.py:102-111), ReduceLROnPlateau, Adam scalars, early stop;
//             per-cluster reduction to dL/dR, dL/dt, backward through the pose head and the output
//             layer(s): its pose row of dL/d(hidden pre-activation)
//   k_bd      two independent roles side by side, told apart by block index:
//             B (bwd2_role)  backward through the hidden layer(s) to the encoder activation, COMPLETE per column block
//                            (a workgroup owns 16 hidden units of the encoder and all H2 rows of their W2 columns), then
//                            those encoder rows' weight gradients + Adam and the NEXT epoch's encoder activation
//             D (dw_role)    hidden / output rows: weight gradients merged with the Adam update (no gradient buffer)
//   k_l2      the NEXT epoch's hidden activation, from B's encoder activation and D's updated hidden rows
//   (k_l1, and k_l2 once more: the first epoch's activations, once per train)
//
// Everything is fp32 like the reference; every reduction has a fixed order (bit-reproducible
// run to run).  State that the reference keeps in Python (min_loss, count, scheduler, lr) lives in
// a double-buffered device struct indexed by epoch parity.
//
// This unit holds the plan, the epoch, graph capture, the chain streams and the public entries; the kernels and their launchers live
// in train_setup.hip (once per train), train_forward.hip (k_l2, k_head), train_nn.hip (NN) and train_backward.hip (k_gradc, k_bd),
// and train_dev.h is what they share.  Nothing here launches a train kernel (only k_spin, the queue probe).
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "train_dev.h"
#include "nn_l1.h"          // nn_grid (the __device__ globals of its measurement builds are read in train_nn.hip, not here)

namespace creg {

constexpr int CHAINS_MAX = 8;       // parallel chains of a batch, in either graph mode

// The plan owns every HIP handle it holds: destroying it is `delete`.
struct Plan {
    creg_train_shape shape{};
    Dims D{};
    Ws W{};
    ParamMap pm[10] = {};         // where the caller's np parameter tensors live in the flat buffer
    int np = 0;
    int B = 1;                    // problems the workspace holds
    size_t bstride = 0;           // bytes between consecutive problems' workspaces
    int branches = 1;             // parallel chains (groups of problems)
    hipGraphExec_t gexec = nullptr;     // one-graph mode (creg_train_shape.graph_branches > 0): `branches` parallel branches of graph_epochs epochs
    bool graph_ready = false;
    int graph_epochs = 0;
    // chain-stream mode (creg_train_shape.graph_branches <= 0): every chain is its OWN linear graph on its OWN stream, forked from /
    // joined to the caller's stream once per train by events -- the chains' hardware queues are then the streams', not what the
    // runtime picks for the branches of one graph at every launch
    bool chain_streams = false;
    hipStream_t cst[CHAINS_MAX] = {};
    hipGraphExec_t cexec[CHAINS_MAX] = {};
    hipEvent_t cfork = nullptr, cjoin[CHAINS_MAX] = {};
    hipStream_t cal_stream = nullptr;   // the caller's stream the chain streams were picked against (pick_chain_streams)
    bool cal_done = false;
    int probe_us = 0;             // pick_chain_streams: the slowest ACCEPTED joint spin of the chain streams with the caller's (150 us kernels: < 250 = concurrent); -1: a chain had to
                                  //   take a stream that shares a hardware queue; 0: not probed (one chain, or the probe is switched off)
    bool target_blocks_valid = false;   // ys4 / ybox hold the k-d leaves of every problem's last run_batch frame (probe / profile overwrite them)

    Plan() = default;
    Plan(const Plan&) = delete;
    Plan& operator=(const Plan&) = delete;
    ~Plan() {
        if (gexec) (void)hipGraphExecDestroy(gexec);
        for (int i = 0; i < CHAINS_MAX; ++i) {        // a chain's stream drains before its graph, join event and the stream itself go
            if (cst[i]) (void)hipStreamSynchronize(cst[i]);
            if (cexec[i]) (void)hipGraphExecDestroy(cexec[i]);
            if (cjoin[i]) (void)hipEventDestroy(cjoin[i]);
            if (cst[i]) (void)hipStreamDestroy(cst[i]);
        }
        if (cfork) (void)hipEventDestroy(cfork);
    }
};

static Slice slice_of(const Plan* P, int first, int count) { return Slice{ws_shift(P->W, (size_t)first * P->bstride), count}; }
// chain gi of P->branches: contiguous groups of B / branches problems, the first B % branches of them one larger
static Slice chain_slice(const Plan* P, int gi) {
    const int q = P->B / P->branches, r = P->B % P->branches;
    return slice_of(P, gi * q + (gi < r ? gi : r), q + (gi < r ? 1 : 0));
}

static bool make_dims(const creg_train_shape* s, Dims* D) {
    if (!s || s->rot < 0 || s->rot > 3 || s->k < 1 || s->k > 256 || (s->hidden != 64 && s->hidden != 128 && s->hidden != 256 && s->hidden != 512) || s->epochs < 1 || s->n_pred < 1 || s->n_tgt < 1 || s->n_pred >= (1ll << 31) ||
        s->n_tgt >= (1ll << 31))
        return false;
    memset(D, 0, sizeof(*D));
    D->rot = s->rot; D->K = s->k; D->KP = (s->k + 19) / 20 * 20; D->H = s->hidden; D->NP = (int)s->n_pred; D->NT = (int)s->n_tgt; D->epochs = s->epochs;
    // model_utils.py: QRegMLP :103-168 (7 inputs x 8 sin / cos features), DQRegMLP :65-101 (ReLU, one decoder), RRegMLP :170-214, RegMLP :216-281
    if (s->rot == ROT_Q) { D->IN = 56; D->HA = D->H / 2; D->HB = D->H; D->OA = 3; D->OB = 4; D->slope = 0.01f; }
    else if (s->rot == ROT_DQ) { D->IN = 64; D->HA = 0; D->HB = D->H; D->OA = 0; D->OB = 8; D->slope = 0.f; }
    else if (s->rot == ROT_6D) { D->IN = 72; D->HA = D->H / 2; D->HB = D->H; D->OA = 3; D->OB = 6; D->slope = 0.01f; }
    else { D->IN = 48; D->HA = D->H / 2; D->HB = D->H; D->OA = 3; D->OB = 3; D->slope = 0.01f; }
    D->H2 = D->HA + D->HB;
    if (!backward_fits(*D)) return false;              // ('6d': K <= 227, <= 193 at hidden 512)
    int o = 0;
    D->oW1 = o; o += D->H * D->IN; D->ob1 = o; o += D->H;
    D->oW2 = o; o += D->H2 * D->H; D->ob2 = o; o += D->H2;
    D->oW3A = o; o += D->OA * D->HA; D->ob3A = o; o += D->OA;
    D->oW3B = o; o += D->OB * D->HB; D->ob3B = o; o += D->OB;
    D->NPAR = o;
    const NnGrid g = nn_grid(D->NP, D->NT, true, true, 4);
    D->nbx = g.blocksA; D->nby = g.blocksB;
    // block-pruned search: 4 queries per wave, a lane holds nbt boxes of the (static) target frame / nbp of the predicted cloud
    // (clusters padded to whole blocks: up to 8 x 64 of them; round 2 stopped at 128 and sent K > 64 at N = 4096 to the
    // exhaustive kernel).  Blocks of 64 points (one per lane and visit) up to 4096 targets, of 256 points (four per lane and
    // visit) beyond: measured at the franka shape (N = 16384, K = 40), 64-point blocks with 4 + 5 boxes per lane take 67.6 us
    // per NN launch against 46 for 64 + 104 blocks of 256 -- evaluating nine boxes per query and lane costs more than the
    // finer blocks save.  The target frame is cut into k-d leaves in LDS, 16384 points per workgroup (k_sort_y; up to four
    // chunks), a cluster by one workgroup (k_sort_p): n_tgt <= 65536, n_pred < 65535 (16-bit indices in the sort keys) and
    // clusters of at most 16384 points are this form's limits; outside them the plan runs the exhaustive kernel per direction.
    // Round 5: nn_search 0 takes sixteen queries per wave (nn_l1_rows) wherever BOTH clouds fit the 64-point block layouts -- up to 256
    // target blocks (four boxes per lane: n_tgt <= 16384, one chunk of k-d leaves) and PS_MAXB blocks of the padded predicted cloud;
    // nn_search 2 = the four-queries-per-wave search of rounds 2-4 (256-point blocks above 4096 targets), nn_search 1 = exhaustive.
    const bool rows_fit = D->NT <= YS_CHUNK && D->NP < 65535 && (D->NP + 63) / 64 + D->K <= PS_MAXB && g.qw == 4;
    // CREG_NN_ROWS: 0 = never, 1 = wherever it fits, unset = where it measured faster (profiles/r05_nn_rows_ab.log)
    const char* rows_env = getenv("CREG_NN_ROWS");
    const bool rows_pays = D->NT > 64 * 64;
    D->rows = s->nn_search == 0 && rows_fit && (rows_env ? rows_env[0] == '1' : rows_pays);
    D->ppl = (D->rows || D->NT <= 64 * 64) ? 1 : 4;
    const int BS = 64 * D->ppl;
    D->nyb = (s->nn_search != 1 && D->NT <= 4 * YS_CHUNK && g.qw == 4) ? (D->NT + BS - 1) / BS : 0;      // (chunks of 16384: k_sort_y)
    D->npb = (D->nyb && D->NP < 65535 && (D->NP + BS - 1) / BS + D->K <= PS_MAXB) ? (D->NP + BS - 1) / BS + D->K : 0;
    const int nt = (D->nyb + 63) / 64, np = (D->npb + 63) / 64;
    D->nbt = nt <= 1 ? 1 : (nt <= 2 ? 2 : 4);
    D->nbp = np <= 2 ? 2 : (np <= 3 ? 3 : (np <= 4 ? 4 : (np <= 5 ? 5 : (np <= 6 ? 6 : 8))));
    if (D->rows) { D->nbx = 4 * D->npb; D->nby = 4 * D->nyb; }          // loss partials per 16-slot group of the query clouds
    return true;
}

static size_t carve(const Dims& D, char* base, Ws* W) {
    size_t o = 0;
    auto take = [&](size_t bytes) -> char* { char* r = base ? base + o : nullptr; o = align_up(o + bytes, 256); return r; };
    const size_t f = sizeof(float);
    Ws w;
    w.P = (float*)take(f * D.NPAR); w.P1 = (float*)take(f * D.NPAR); w.AM = (float*)take(f * D.NPAR); w.AV = (float*)take(f * D.NPAR);
    w.pose_in = (float*)take(f * POSE_IN * D.K); w.enc = (float*)take(f * D.K * D.IN);
    w.x1[0] = (float*)take(f * D.KP * D.H); w.x1[1] = (float*)take(f * D.KP * D.H);
    w.h2[0] = (float*)take(f * D.KP * D.H2); w.h2[1] = (float*)take(f * D.KP * D.H2); w.head_save = (float*)take(f * 16 * D.K);
    w.m2 = (float*)take(f * 16 * D.K); w.gm2 = (float*)take(f * 16 * D.K);
    w.pts4 = (float4*)take(sizeof(float4) * D.NP); w.y4 = (float4*)take(sizeof(float4) * D.NT);
    w.pred4 = (float4*)take(sizeof(float4) * D.NP);
    const size_t bs = 64 * (size_t)D.ppl;
    w.ys4 = (float4*)take(sizeof(float4) * bs * (D.nyb ? D.nyb : 1)); w.ybox = (float*)take(f * 6 * 64 * D.nbt);
    w.psl4 = (float4*)take(sizeof(float4) * bs * (D.npb ? D.npb : 1)); w.ps4 = (float4*)take(sizeof(float4) * bs * (D.npb ? D.npb : 1));
    w.pbox = (float*)take(f * 6 * 64 * D.nbp); w.sb = (int*)take(sizeof(int) * (D.K + 1));
    w.sgn_x = (int*)take(sizeof(int) * D.NP);
    w.cnt4 = (int4*)take(sizeof(int4) * D.NP);
    w.lossp_x = (float*)take(f * D.nbx); w.lossp_y = (float*)take(f * D.nby);
    w.g_out = (float*)take(f * 16 * D.KP); w.g_h2 = (float*)take(f * D.KP * D.H2);
    w.state = (TrainState*)take(sizeof(TrainState) * 2);
    w.bc1 = (double*)take(sizeof(double) * (D.epochs + 1)); w.bc2s = (float*)take(f * (D.epochs + 1));
    w.best_m = (float*)take(f * 16 * D.K); w.best_pred = (float*)take(f * 3 * D.NP);
    w.loss_hist = (float*)take(f * D.epochs); w.lr_hist = (float*)take(f * D.epochs); w.result = (float*)take(f * 4);
    w.off = (int*)take(sizeof(int) * (D.K + 1)); w.hyper = (Hyper*)take(sizeof(Hyper));
    w.ysum = (unsigned long long*)take(sizeof(unsigned long long) * 4);
    if (W) *W = w;
    return o;
}
constexpr int NKERN = 5;
// `ev` (optional): NKERN + 1 events recorded before kernel 0 and after each kernel.
// Entering epoch e, x1[e & 1] and h2[e & 1] hold the activations of the current parameters (k_l1 / k_l2 for epoch 0,
// k_bd's B role / k_l2 of the previous epoch afterwards).
static void enqueue_epoch(const Plan* P, const Slice& S, int epoch, hipStream_t s, hipEvent_t* ev = nullptr) {
    const Dims& D = P->D;
    const int par = epoch & 1;
    auto mark = [&](int i) { if (ev) (void)hipEventRecord(ev[i], s); };
    mark(0);
    launch_head(D, S, P->bstride, par, s); mark(1);
    launch_nn(D, S, P->bstride, par, s); mark(2);
    launch_gradc(D, S, P->bstride, epoch, s); mark(3);
    launch_bd(D, S, P->bstride, epoch, s); mark(4);
    launch_l2(D, S, P->bstride, par ^ 1, s); mark(5);        // the next epoch's hidden activation: next encoder activation (B) x updated hidden rows (D)
}

}  // namespace creg
using namespace creg;

// EPG consecutive epochs captured as one graph (G independent branches over contiguous groups of problems).  On any
// failure the capture is ended; every stream / event / graph created here is released when the function returns.
static int capture_epochs(Plan* P, int epg) {
    // captured on a private stream (torch's current stream is usually the null stream, which cannot be captured); the
    // instantiated graph is then launched on the caller's stream.
    const int G = P->branches;
    ScopedStream cs, cs2[CHAINS_MAX];
    ScopedEvents ev(CHAINS_MAX);                             // [0]: the fork, [gi]: the join of branch gi
    hipEvent_t& ef = ev[0];
    hipEvent_t* ej = ev.v.data();
    ScopedGraph g;
    FirstError fe;
    CREG_TRY(fe, hipStreamCreateWithFlags(&cs.h, hipStreamNonBlocking));
    CREG_TRY(fe, hipStreamBeginCapture(cs.h, hipStreamCaptureModeThreadLocal));
    const bool capturing = fe.ok();
    if (G > 1) {
        // fork / join through events, so the instantiated graph has parallel chains: the runtime feeds them to
        // different hardware queues and the latency-bound kernels of one group overlap the long launches of the
        // other.  Problems never interact, so results do not depend on G (stress-tested: tests/test_gpu_parity.py).
        CREG_TRY(fe, hipEventCreateWithFlags(&ef, hipEventDisableTiming));
        CREG_TRY(fe, hipEventRecord(ef, cs.h));
    }
    for (int gi = 0; gi < G && fe.ok(); ++gi) {
        hipStream_t st = cs.h;
        if (gi > 0) {
            CREG_TRY(fe, hipStreamCreateWithFlags(&cs2[gi].h, hipStreamNonBlocking));
            CREG_TRY(fe, hipStreamWaitEvent(cs2[gi].h, ef, 0));
            st = cs2[gi].h;
        }
        if (!fe.ok()) break;
        const Slice S = chain_slice(P, gi);
        for (int i = 0; i < epg; ++i) enqueue_epoch(P, S, i, st);
        if (gi > 0) {
            CREG_TRY(fe, hipEventCreateWithFlags(&ej[gi], hipEventDisableTiming));
            CREG_TRY(fe, hipEventRecord(ej[gi], st));
        }
    }
    for (int gi = 1; gi < G; ++gi) if (ej[gi]) CREG_TRY(fe, hipStreamWaitEvent(cs.h, ej[gi], 0));
    if (capturing) fe.note(hipStreamEndCapture(cs.h, &g.h), "hipStreamEndCapture");      // always end the capture, also after a failure
    CREG_TRY(fe, hipGraphInstantiate(&P->gexec, g.h, nullptr, nullptr, 0));
    if (!fe.ok()) {
        (void)hipGetLastError();
        if (P->gexec) { (void)hipGraphExecDestroy(P->gexec); P->gexec = nullptr; }
        creg::set_error("creg_train_plan_run_batch: graph capture failed: %s: %s", fe.what, hipGetErrorString(fe.err));
        return CREG_EHIP;
    }
    P->graph_ready = true;
    P->graph_epochs = epg;
    return CREG_OK;
}

// ---- chain streams must sit in DIFFERENT hardware queues (round 5) -------------------------------------------------------------
// The runtime multiplexes streams onto GPU_MAX_HW_QUEUES (4) hardware queues: the first four streams of a process get a queue each,
// every later one SHARES the queue with the fewest users -- possibly the caller's.  Two chains in one queue run one after the other
// (75 us per epoch instead of 45.8: the default bench line fell 182 -> 112 frames/s the moment a world-1 RCCL group, which owns
// streams of its own, was created before the plan; profiles/r05_rccl_vs_chains.log).  HIP does not say which queue a stream got, so
// it is measured: a stream is accepted as a chain's when a 150 us spin kernel on it runs CONCURRENTLY with one on the caller's stream
// and on the chains picked before it; rejected candidates stay alive until the pick is over (so that the next one lands elsewhere).
__global__ void k_spin(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
constexpr unsigned long long SPIN_TICKS = 15000;        // wall_clock64 runs at 100 MHz: 150 us
constexpr double SPIN_TOGETHER_US = 250.0;              // a joint spin below this ran concurrently

static double spin_together_us(hipStream_t* st, int n) {
    for (int i = 0; i < n; ++i) if (hipStreamSynchronize(st[i]) != hipSuccess) return -1.0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n; ++i) hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, st[i], SPIN_TICKS);
    if (hipGetLastError() != hipSuccess) return -1.0;
    for (int i = 0; i < n; ++i) if (hipStreamSynchronize(st[i]) != hipSuccess) return -1.0;
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}
// The joint spin of a candidate (the last of `st`) with the streams it has to overlap; a late host thread looks like a shared
// queue, so a slow (or failed) measurement is taken once more and the smaller one counts.  Negative: no measurement.
static double candidate_spin_us(hipStream_t* st, int n) {
    double t = spin_together_us(st, n);
    if (t < 0 || t >= SPIN_TOGETHER_US) {
        const double t2 = spin_together_us(st, n);
        if (t2 >= 0 && (t < 0 || t2 < t)) t = t2;
    }
    return t;
}

// (Re)creates P->cst[1 .. branches-1] so that they overlap with `s` and with each other; keeps what it has when no better stream exists.
static int pick_chain_streams(Plan* P, hipStream_t s) {
    static const bool probe = !(getenv("CREG_NO_QUEUE_PROBE") && getenv("CREG_NO_QUEUE_PROBE")[0] == '1');
    constexpr int ATTEMPTS = 7;
    P->probe_us = 0;
    auto fits = [](double t) { return t >= 0 && t < SPIN_TOGETHER_US; };
    auto accept = [&](double t) { if (P->probe_us >= 0 && (int)t > P->probe_us) P->probe_us = (int)t; };
    for (int gi = 1; gi < P->branches; ++gi) {
        hipStream_t set[CHAINS_MAX + 1], rejected[ATTEMPTS + 1];
        int ns = 0, nr = 0;
        set[ns++] = s;
        for (int j = 1; j < gi; ++j) set[ns++] = P->cst[j];
        hipStream_t chosen = nullptr;
        if (P->cst[gi]) {                                    // the stream of an earlier pick (another caller stream): keep it if it still fits
            set[ns] = P->cst[gi];
            const double t = candidate_spin_us(set, ns + 1);
            if (!probe || fits(t)) { chosen = P->cst[gi]; if (probe) accept(t); }
            else { (void)hipStreamSynchronize(P->cst[gi]); rejected[nr++] = P->cst[gi]; P->cst[gi] = nullptr; }
        }
        for (int attempt = 0; !chosen && attempt < ATTEMPTS; ++attempt) {
            hipStream_t cs = nullptr;
            if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) break;
            if (!probe) { chosen = cs; break; }
            set[ns] = cs;
            const double t = candidate_spin_us(set, ns + 1);
            if (fits(t)) { chosen = cs; accept(t); }
            else rejected[nr++] = cs;
        }
        if (!chosen && nr) { chosen = rejected[--nr]; P->probe_us = -1; }      // every queue is shared with somebody: any stream is as good as another
        for (int i = 0; i < nr; ++i) (void)hipStreamDestroy(rejected[i]);
        if (!chosen) {
            (void)hipGetLastError();
            creg::set_error("creg_train_plan_run_batch: cannot create a stream for chain %d", gi);
            return CREG_EHIP;
        }
        P->cst[gi] = chosen;
    }
    P->cal_stream = s; P->cal_done = true;
    return CREG_OK;
}

// chain-stream mode: chain gi's EPG epochs as a linear graph (captured on a temporary stream: an instantiated graph runs on any)
static int capture_chains(Plan* P, int epg) {
    FirstError fe;
    if (!P->cfork) CREG_TRY(fe, hipEventCreateWithFlags(&P->cfork, hipEventDisableTiming));
    ScopedStream cs;
    CREG_TRY(fe, hipStreamCreateWithFlags(&cs.h, hipStreamNonBlocking));
    for (int gi = 0; gi < P->branches && fe.ok(); ++gi) {
        ScopedGraph g;
        if (gi > 0 && !P->cjoin[gi]) CREG_TRY(fe, hipEventCreateWithFlags(&P->cjoin[gi], hipEventDisableTiming));
        if (P->cexec[gi]) { (void)hipGraphExecDestroy(P->cexec[gi]); P->cexec[gi] = nullptr; }      // (a retry after a failed capture)
        CREG_TRY(fe, hipStreamBeginCapture(cs.h, hipStreamCaptureModeThreadLocal));
        if (fe.ok()) {
            const Slice S = chain_slice(P, gi);
            for (int i = 0; i < epg; ++i) enqueue_epoch(P, S, i, cs.h);
            fe.note(hipStreamEndCapture(cs.h, &g.h), "hipStreamEndCapture");
        }
        CREG_TRY(fe, hipGraphInstantiate(&P->cexec[gi], g.h, nullptr, nullptr, 0));
    }
    if (!fe.ok()) {
        (void)hipGetLastError();
        for (int gi = 0; gi < CHAINS_MAX; ++gi) if (P->cexec[gi]) { (void)hipGraphExecDestroy(P->cexec[gi]); P->cexec[gi] = nullptr; }
        creg::set_error("creg_train_plan_run_batch: chain graph capture failed: %s: %s", fe.what, hipGetErrorString(fe.err));
        return CREG_EHIP;
    }
    P->graph_ready = true;
    P->graph_epochs = epg;
    return CREG_OK;
}

// chain-stream mode, the whole train: fork once, every chain runs it on its own stream (graph replays, then the epochs that do not
// fill a graph), join once.  Chain 0 runs on the CALLER's stream: a stream that only waits for the others would hold a barrier
// packet in its hardware queue for the whole train, and a parked barrier slows the chains in the other queues by ~10 %
// (measured, tests/measure/frame_phases_by_chains.py).
static int run_chains(Plan* P, hipStream_t s) {
    const Dims& D = P->D;
    if (P->branches > 1 && (!P->cal_done || P->cal_stream != s))
        if (int rc = pick_chain_streams(P, s)) return rc;      // streams in hardware queues of their own (measured, see there)
    auto st_of = [&](int gi) { return gi == 0 ? s : P->cst[gi]; };
    FirstError fe;
    CREG_TRY(fe, hipEventRecord(P->cfork, s));
    for (int gi = 1; gi < P->branches; ++gi) CREG_TRY(fe, hipStreamWaitEvent(P->cst[gi], P->cfork, 0));
    int e = 0;
    for (; fe.ok() && e + P->graph_epochs <= D.epochs; e += P->graph_epochs)
        for (int gi = 0; gi < P->branches; ++gi) CREG_TRY(fe, hipGraphLaunch(P->cexec[gi], st_of(gi)));
    for (int gi = 0; fe.ok() && gi < P->branches; ++gi) {
        const Slice S = chain_slice(P, gi);
        for (int e2 = e; e2 < D.epochs; ++e2) enqueue_epoch(P, S, e2, st_of(gi));
    }
    // the join is enqueued ALSO after a failure: chains that did start must not be left running on the workspace, un-joined,
    // beside whatever the caller does next (a retry would stage inputs under them)
    for (int gi = 1; gi < P->branches; ++gi) {
        if (hipEventRecord(P->cjoin[gi], P->cst[gi]) != hipSuccess || hipStreamWaitEvent(s, P->cjoin[gi], 0) != hipSuccess) {
            (void)hipStreamSynchronize(P->cst[gi]);
            fe.note(hipErrorUnknown, "joining a chain stream");
        }
    }
    if (!fe.ok()) {
        (void)hipGetLastError();
        creg::set_error("creg_train_plan_run_batch: %s: %s", fe.what, hipGetErrorString(fe.err));
        return CREG_EHIP;
    }
    return CREG_OK;
}

// ---- what the entries share ----------------------------------------------------------------------------------------------------
// How run_batch, resume, probe and profile begin: EVERY problem's pointers are checked before the first launch, then the inputs are
// staged, then the two clouds are cut into k-d leaves.  Only run_batch may keep the target frame's leaves of its previous run (when
// the caller vouches for every problem's frame; the launch verifies the claim -- see k_sort_y); the other three overwrite them.
static int begin_run(const char* who, Plan* P, const Slice& S, const creg_train_args* args, bool with_outputs, bool may_keep_leaves,
                     hipStream_t s) {
    bool keep = may_keep_leaves && P->target_blocks_valid;
    for (int b = 0; b < S.nz; ++b) {
        const creg_train_args* a = args + b;
        CREG_REQUIRE(a->m && a->y && a->local_pts && a->seg_offsets && a->params && (!with_outputs || (a->best_m && a->best_pred && a->result)),
                     "%s: null pointer in problem %d", who, b);
        for (int i = 0; i < P->np; ++i) CREG_REQUIRE(a->params[i], "%s: params[%d] of problem %d is null", who, i, b);
        keep = keep && a->y_unchanged != 0;
    }
    if (int rc = stage_inputs(P->D, S, P->bstride, args, s)) return rc;
    launch_sorts(P->D, S, P->bstride, s, keep);
    P->target_blocks_valid = may_keep_leaves;
    return CREG_OK;
}

// How run_batch and resume end: the results of slice S's problems and their parameters back into the callers' tensors (`T` may
// already hold ranges of the entry's own).
static void results_out(const Plan* P, const Slice& S, const creg_train_args* args, CopyTable& T, hipStream_t s) {
    const Dims& D = P->D;
    for (int b = 0; b < S.nz; ++b) {
        const creg_train_args* a = args + b;
        const Ws W = ws_shift(S.W, (size_t)b * P->bstride);
        for (int i = 0; i < P->np; ++i) copy_table_add(T, W.P + P->pm[i].off, a->params[i], sizeof(float) * P->pm[i].count, s);
        copy_table_add(T, W.best_m, a->best_m, sizeof(float) * 16 * D.K, s);
        copy_table_add(T, W.best_pred, a->best_pred, sizeof(float) * 3 * D.NP, s);
        copy_table_add(T, W.result, a->result, sizeof(float) * 4, s);
        if (a->loss_hist) copy_table_add(T, W.loss_hist, a->loss_hist, sizeof(float) * D.epochs, s);
        if (a->lr_hist) copy_table_add(T, W.lr_hist, a->lr_hist, sizeof(float) * D.epochs, s);
    }
    copy_table_launch(T, s);
}

static int batch_of(const creg_train_shape* s) { return s->batch >= 1 ? s->batch : 1; }

extern "C" size_t creg_train_workspace_bytes(const creg_train_shape* shape) {
    Dims D;
    if (!make_dims(shape, &D) || shape->batch < 0 || shape->batch > BATCH_MAX) return 0;
    return align_up(carve(D, nullptr, nullptr), 256) * batch_of(shape);
}

extern "C" int creg_train_plan_create(const creg_train_shape* shape, void* workspace, size_t workspace_bytes,
                                      creg_train_plan** plan) {
    Dims D;
    CREG_REQUIRE(plan && workspace, "creg_train_plan_create: null pointer");
    CREG_REQUIRE(make_dims(shape, &D), "creg_train_plan_create: unsupported shape (rot in 0..3, hidden in {64, 128, 256, 512}, 1 <= k <= 256 with the K x IN features + the B role's tiles inside 160 KB of LDS, sizes >= 1)");
    CREG_REQUIRE(((uintptr_t)workspace & 255) == 0, "creg_train_plan_create: workspace must be 256-byte aligned");
    CREG_REQUIRE(shape->batch >= 0 && shape->batch <= BATCH_MAX, "creg_train_plan_create: batch must be in [0, %d]", BATCH_MAX);
    const size_t one = align_up(carve(D, nullptr, nullptr), 256), need = one * batch_of(shape);
    CREG_REQUIRE(workspace_bytes >= need, "creg_train_plan_create: workspace too small (%zu < %zu)", workspace_bytes, need);
    auto P = std::make_unique<Plan>();       // (released to the caller on success only: every return below frees it)
    P->shape = *shape; P->D = D; P->np = param_map(D, P->pm);
    carve(D, (char*)workspace, &P->W);
    P->B = batch_of(shape); P->bstride = one;
    // How the problems of a batch share the GPU (round 4, profiles/r04_chains_by_batch.log; bench.py --graph-branches):
    //   graph_branches < 0: -n CHAIN STREAMS -- the batch is cut into n contiguous groups, every group's epochs are a LINEAR graph
    //     (replayed from pre-built packets: 0.6-1.2 ms of host time per 300-epoch train) on its own stream; chain 0 uses the
    //     caller's stream, the others fork from / join it once per train.
    //   graph_branches > 0: n parallel branches inside ONE graph (rounds 2-3).  The runtime enqueues every node of a multi-branch
    //     graph from the host at each replay -- 9 ms per train with two branches, 14 of the train's 15 ms with three, which is why
    //     three branches ran "bimodal" (host-bound: any hiccup of the enqueuing thread stalls a queue).
    //   0 = auto: chain streams; one chain up to 4 problems (47.9 / 92.9 / 127 / 153 frames/s for 1-4 sequences against
    //     - / 84 / 119 / 152 with two), two for 5-7 (182 / 201 / 219 against 175 / 188 / 189 with one and 172 / 198 / 209 with
    //     three), three from 8 (230 against 226); frames above 4096 points (several points per lane in the NN kernels, whose tails
    //     leave CUs idle) take three from 3 problems on (franka shape 79.4 against 74.8 / 74.0 with two / one).  Four chains need a
    //     fifth hardware queue and collapse (112 at 6 sequences).  Results never depend on any of this.
    const int auto_chains = (D.NT > 64 * 64 && P->B >= 3) ? 3 : (P->B >= 8 ? 3 : (P->B >= 5 ? 2 : 1));
    P->chain_streams = shape->graph_branches <= 0;
    P->branches = shape->graph_branches > 0 ? shape->graph_branches : (shape->graph_branches < 0 ? -shape->graph_branches : auto_chains);
    if (P->branches > P->B) P->branches = P->B;
    if (P->branches > CHAINS_MAX) P->branches = CHAINS_MAX;
    if (int rc = bd_raise_lds(D)) return rc;
    if (int rc = setup_raise_lds(D)) return rc;
    *plan = (creg_train_plan*)P.release();
    return CREG_OK;
}

extern "C" int creg_train_plan_run_batch(creg_train_plan* plan, const creg_train_args* args, int32_t n,
                                         creg_stream_t stream) {
    Plan* P = (Plan*)plan;
    CREG_REQUIRE(P && args, "creg_train_plan_run_batch: null pointer");
    CREG_REQUIRE(n == P->B, "creg_train_plan_run_batch: the plan was created for a batch of %d problems, got %d", P->B, n);
    hipStream_t s = (hipStream_t)stream;
    const Dims& D = P->D;
    const Slice all = slice_of(P, 0, P->B);
    if (int rc = begin_run("creg_train_plan_run_batch", P, all, args, true, true, s)) return rc;
    int e = 0;
    if (P->shape.use_graph && D.epochs >= 2) {
        // One graph holds EPG consecutive epochs (even count: the epoch number enters the kernels only
        // through its parity, the history index comes from the device-side counter state.epochs_run),
        // so a 300-epoch train is 6 graph launches instead of 1800 kernel launches.
        int epg = P->shape.use_graph > 1 ? P->shape.use_graph : 50;
        if (epg > D.epochs) epg = D.epochs;
        epg &= ~1;
        if (!P->graph_ready) {
            const int rc = P->chain_streams ? capture_chains(P, epg) : capture_epochs(P, epg);
            if (rc) return rc;
        }
        if (P->chain_streams) {
            if (int rc = run_chains(P, s)) { P->target_blocks_valid = false; return rc; }      // nothing of this run may be vouched for by the next one
            e = D.epochs;
        } else {
            for (; e + P->graph_epochs <= D.epochs; e += P->graph_epochs) CREG_HIP(hipGraphLaunch(P->gexec, s));
        }
    }
    for (; e < D.epochs; ++e) enqueue_epoch(P, all, e, s);
    launch_params_home(D, all, P->bstride, D.epochs & 1, 0, s);
    CREG_LAUNCH_CHECK();
    CopyTable T;
    results_out(P, all, args, T, s);
    return CREG_OK;
}

extern "C" int creg_train_plan_run(creg_train_plan* plan, const creg_train_args* a, creg_stream_t stream) {
    return creg_train_plan_run_batch(plan, a, 1, stream);
}

// Round 6: a train continued from a caller-supplied optimizer / control state (torch.optim.Adam's exp_avg / exp_avg_sq / step,
// ReduceLROnPlateau's best / num_bad_epochs / lr, train()'s min_loss / count: mlp_reg.py:41-50,96-119) -- checkpoint / resume of a
// train, and what the teacher-forced late-epoch parity tests are built on (the oracle's state entering epoch e, ONE epoch of the plan).
// Problem slot 0, eager launches (the kernels are the graph's; graph == eager is tested elsewhere).
extern "C" int creg_train_plan_resume(creg_train_plan* plan, const creg_train_args* a, const creg_train_state* from, int32_t n_epochs,
                                      float* const* exp_avg_out, float* const* exp_avg_sq_out, double* state_out, creg_stream_t stream) {
    Plan* P = (Plan*)plan;
    CREG_REQUIRE(P && a && from, "creg_train_plan_resume: null pointer");
    CREG_REQUIRE(from->exp_avg && from->exp_avg_sq, "creg_train_plan_resume: the state needs both Adam moment arrays");
    const Dims& D = P->D;
    CREG_REQUIRE(n_epochs >= 1 && from->step >= 0 && from->epochs_run >= 0 && from->step + n_epochs <= D.epochs && from->epochs_run + n_epochs <= D.epochs,
                 "creg_train_plan_resume: step %d / epochs_run %d + %d epochs exceed the plan's %d", from->step, from->epochs_run, n_epochs, D.epochs);
    CREG_REQUIRE(from->lr >= 0.0 && from->sched_bad >= 0 && from->count >= 0, "creg_train_plan_resume: negative lr or counter");
    const ParamMap* pm = P->pm;
    const int np = P->np;
    for (int i = 0; i < np; ++i) CREG_REQUIRE(from->exp_avg[i] && from->exp_avg_sq[i], "creg_train_plan_resume: moment tensor %d is null", i);
    hipStream_t s = (hipStream_t)stream;
    const Slice one = slice_of(P, 0, 1);
    // parameters into the parity-0 buffer, the activations of epoch "0" from them, state and moments zeroed
    if (int rc = begin_run("creg_train_plan_resume", P, one, a, true, false, s)) return rc;
    CopyTable T;
    for (int i = 0; i < np; ++i) {
        copy_table_add(T, from->exp_avg[i], P->W.AM + pm[i].off, sizeof(float) * pm[i].count, s);
        copy_table_add(T, from->exp_avg_sq[i], P->W.AV + pm[i].off, sizeof(float) * pm[i].count, s);
    }
    if (from->best_epoch >= 0) {            // the best so far is the caller's (kept when none of the resumed epochs improves on min_loss)
        copy_table_add(T, a->best_m, P->W.best_m, sizeof(float) * 16 * D.K, s);
        copy_table_add(T, a->best_pred, P->W.best_pred, sizeof(float) * 3 * D.NP, s);
    }
    copy_table_launch(T, s);
    launch_set_state(D, P->W, *from, s);
    for (int e = 0; e < n_epochs; ++e) enqueue_epoch(P, one, e, s);
    launch_params_home(D, one, P->bstride, n_epochs & 1, from->step, s);
    if (state_out) launch_get_state(P->W, n_epochs & 1, state_out, s);
    CREG_LAUNCH_CHECK();
    for (int i = 0; i < np; ++i) {          // the moments as well, where the caller asks for them
        if (exp_avg_out && exp_avg_out[i]) copy_table_add(T, P->W.AM + pm[i].off, exp_avg_out[i], sizeof(float) * pm[i].count, s);
        if (exp_avg_sq_out && exp_avg_sq_out[i]) copy_table_add(T, P->W.AV + pm[i].off, exp_avg_sq_out[i], sizeof(float) * pm[i].count, s);
    }
    results_out(P, one, a, T, s);
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

extern "C" int creg_train_plan_probe(creg_train_plan* plan, const creg_train_args* a, float* m2, float* pred,
                                     float* loss, float* grad_m2, creg_stream_t stream) {
    Plan* P = (Plan*)plan;
    CREG_REQUIRE(P && a, "creg_train_plan_probe: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const Dims& D = P->D; const Ws& W = P->W;
    const Slice one = slice_of(P, 0, 1);
    if (int rc = begin_run("creg_train_plan_probe", P, one, a, false, false, s)) return rc;
    launch_head(D, one, P->bstride, 0, s);
    launch_nn(D, one, 0, 0, s);
    launch_gradc(D, one, 0, 0, s);
    CREG_LAUNCH_CHECK();
    if (m2) CREG_HIP(hipMemcpyAsync(m2, W.m2, sizeof(float) * 16 * D.K, hipMemcpyDeviceToDevice, s));
    if (pred) CREG_HIP(hipMemcpyAsync(pred, W.best_pred, sizeof(float) * 3 * D.NP, hipMemcpyDeviceToDevice, s));
    if (loss) CREG_HIP(hipMemcpyAsync(loss, W.loss_hist, sizeof(float), hipMemcpyDeviceToDevice, s));
    if (grad_m2) CREG_HIP(hipMemcpyAsync(grad_m2, W.gm2, sizeof(float) * 16 * D.K, hipMemcpyDeviceToDevice, s));
    return CREG_OK;
}

extern "C" int creg_train_plan_profile(creg_train_plan* plan, const creg_train_args* a, int32_t n_epochs,
                                       float* us_out, creg_stream_t stream) {
    Plan* P = (Plan*)plan;
    CREG_REQUIRE(P && a && us_out && n_epochs >= 1, "creg_train_plan_profile: bad argument");
    hipStream_t s = (hipStream_t)stream;
    // the launches as the timed region issues them: the problems of the first (largest) graph branch in grid.z, EVERY one of them
    // staged from `a` and advanced through the bracketed epochs.  (Until the end of round 3 only problem 0 was staged: the others
    // kept the state of the caller's last trains, and a train that had stopped early leaves `stopped` set -- its workgroups in the
    // back-to-back launches below requested their loads and returned, so those launches carried less work than their label said.)
    const int br = P->shape.use_graph ? P->branches : 1;
    const int nzb = P->B / br + (P->B % br ? 1 : 0);
    std::vector<creg_train_args> all((size_t)nzb, *a);
    const Slice S = slice_of(P, 0, nzb);
    if (int rc = begin_run("creg_train_plan_profile", P, S, all.data(), false, false, s)) return rc;
    ScopedEvents ev((size_t)(NKERN + 1) * n_epochs);
    for (auto& e : ev.v) CREG_HIP(hipEventCreate(&e));
    for (int e = 0; e < n_epochs; ++e) enqueue_epoch(P, S, e, s, ev.v.data() + (NKERN + 1) * e);
    CREG_LAUNCH_CHECK();
    CREG_HIP(hipStreamSynchronize(s));
    double acc[NKERN] = {0};
    for (int e = 0; e < n_epochs; ++e)
        for (int k = 0; k < NKERN; ++k) {
            float ms = 0.f;
            CREG_HIP(hipEventElapsedTime(&ms, ev[(NKERN + 1) * e + k], ev[(NKERN + 1) * e + k + 1]));
            acc[k] += ms;
        }
    us_out[0] = 0.f;                    // (round 2's k_l2 slot: the hidden forward has no launch of its own any more)
    for (int k = 0; k < NKERN; ++k) us_out[1 + k] = (float)(acc[k] * 1000.0 / n_epochs);
    // us_out[6], us_out[8..11]: one launch alone, REP back-to-back launches between two events (per-kernel event brackets carry
    // ~7 us of event overhead; this one carries only the launch-to-launch gap, so it upper-bounds the rocprofv3 kernel duration by
    // ~1 us): the nearest-neighbour launch, then k_bd, k_l2, k_head, k_gradc (measurement hooks: every k_bd launch is one more Adam
    // step on the plan's copies of the parameters, alternating between the two buffers; the caller's tensors are not written back)
    const int REP = 200;
    const Dims& D = P->D;
    auto b2b = [&](auto launch, float* out) -> int {
        float ms = 0.f;
        CREG_HIP(hipEventRecord(ev[0], s));
        for (int i = 0; i < REP; ++i) launch(i);
        CREG_HIP(hipEventRecord(ev[1], s));
        CREG_HIP(hipStreamSynchronize(s));
        CREG_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        *out = ms * 1000.f / REP;
        return CREG_OK;
    };
    if (int rc = b2b([&](int) { launch_nn(D, S, P->bstride, 0, s); }, us_out + 6)) return rc;
    us_out[7] = (float)S.nz;        // problems carried by that launch
    if (int rc = bd_stamps_arm(true)) return rc;
    if (int rc = b2b([&](int i) { launch_bd(D, S, P->bstride, i, s); }, us_out + 8)) return rc;
    if (int rc = bd_stamps_arm(false)) return rc;
    if (int rc = b2b([&](int i) { launch_l2(D, S, P->bstride, i & 1, s); }, us_out + 9)) return rc;
    if (int rc = b2b([&](int i) { launch_head(D, S, P->bstride, i & 1, s); }, us_out + 10)) return rc;
    if (int rc = b2b([&](int i) { launch_gradc(D, S, P->bstride, i, s); }, us_out + 11)) return rc;
    CREG_LAUNCH_CHECK();
    return CREG_OK;
}

extern "C" int creg_train_plan_info(const creg_train_plan* plan, creg_train_plan_info_t* info) {
    CREG_REQUIRE(plan && info, "creg_train_plan_info: null pointer");
    const Plan* P = (const Plan*)plan;
    info->pruned_target_search = P->D.rows ? 2 : (P->D.nyb > 0);
    info->pruned_predicted_search = P->D.npb > 0;
    info->graph_branches = P->branches;
    info->batch = P->B;
    info->epochs_per_graph = P->shape.use_graph ? P->graph_epochs : 0;
    info->nn_points_per_lane = P->D.ppl;
    info->nn_boxes_target = P->D.nbt;
    info->nn_boxes_predicted = P->D.nbp;
    info->chain_probe_us = P->probe_us;
    return CREG_OK;
}

extern "C" int creg_train_plan_destroy(creg_train_plan* plan) {
    delete (Plan*)plan;
    return CREG_OK;
}
