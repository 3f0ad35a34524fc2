// train_nn.hip -- the train plan's nearest-neighbour launch: Chamfer's two L1 searches with the loss partials and the sign scatter
// as the epilogue (k_nn_rows, k_nn_plan or nn_l1.h's k_nn_l1 by problem size: launch_nn), and the read-backs of its measurement builds.
#include <type_traits>
#include <vector>
#include "train_dev.h"
#include "nn_l1.h"

namespace creg {

// ------------------------------------------------------------------------------------------ NN epilogue
// Runs inside the nearest-neighbour launch (results are final there): sign bits of the x->y term,
// integer sign scatter of the y->x term (exact, order independent), per-block loss partials.
struct EngineEpi {
    int* sgn_x; int4* cnt4; float* lossp_x; float* lossp_y;
    size_t bstride;
    const int* stopped;            // &state[epoch & 1].stopped of problem 0
    __device__ __forceinline__ void shift(int z) {
        const size_t b = (size_t)z * bstride;
        sgn_x = (int*)((char*)sgn_x + b); cnt4 = (int4*)((char*)cnt4 + b);
        lossp_x = (float*)((char*)lossp_x + b); lossp_y = (float*)((char*)lossp_y + b);
        stopped = (const int*)((const char*)stopped + b);
    }
    __device__ __forceinline__ void operator()(int dir, int q, int idx, float d, float qx, float qy, float qz,
                                               float tx, float ty, float tz, float& acc) const {
        if (dir == 0) {          // query pred[q], nearest y[idx]: knn(p1=x,p2=y) grad_p1 sign = (p1 > p2 ? +1 : -1)
            sgn_x[q] = (qx > tx ? 1 : 0) | (qy > ty ? 2 : 0) | (qz > tz ? 4 : 0);
        } else {                 // query y[q], nearest pred[idx]: knn(p1=y,p2=x) grad_p2 -= sign
            atomicAdd(&cnt4[idx].x, (qx > tx) ? -1 : 1);
            atomicAdd(&cnt4[idx].y, (qy > ty) ? -1 : 1);
            atomicAdd(&cnt4[idx].z, (qz > tz) ? -1 : 1);
        }
        acc += d;
    }
    __device__ __forceinline__ void finish(int dir, int blk, float s, float*) const { (dir == 0 ? lossp_x : lossp_y)[blk] = s; }
};

// The plan's nearest-neighbour launch: blocks of direction 0 search the block-sorted target frame for the predicted
// points (pruned, exact); direction 1 searches the predicted cloud for the target points -- over k_head's
// block-sorted copy of it (P1) or exhaustively.  Same epilogue, same per-block loss partials as k_nn_l1: the
// launches are interchangeable bit for bit.
template <bool P1, int PPL, int NBT, int NBP>
__global__ __launch_bounds__(NN_BLOCK) void k_nn_plan(const float* A, int na, const float* B, int nb, int blocksA,
                                                      int blocksB, EngineEpi epi, NnBlocks yb, NnBlocks pb, size_t zstride) {
    // grid.x = (blocksA + blocksB) * problems, direction 1 (the long blocks when it is exhaustive) of ALL problems
    // first: the dispatcher hands workgroups out in index order, so the long ones spread over the CUs before the
    // short ones fill in
    // every kernel argument in the entry block, one wait (see k_bd)
    asm volatile("" :: "s"(A), "s"(na), "s"(B), "s"(nb), "s"(blocksA), "s"(blocksB), "s"(epi.sgn_x), "s"(epi.cnt4), "s"(epi.lossp_x), "s"(epi.lossp_y),
                 "s"(epi.bstride), "s"(epi.stopped), "s"(yb.ts4), "s"(yb.tbox), "s"(yb.nblk), "s"(pb.ts4), "s"(pb.tbox), "s"(pb.nblk_dev), "s"(zstride));
    const int nz = gridDim.x / (blocksA + blocksB);
    int i = blockIdx.x, z, bx;
    if (i < blocksB * nz) { z = i / blocksB; bx = blocksA + (i - z * blocksB); }
    else { i -= blocksB * nz; z = i / blocksA; bx = i - z * blocksA; }
    const size_t zb = z * zstride;
    A = (const float*)((const char*)A + zb);
    B = (const float*)((const char*)B + zb);
    yb.ts4 = (const float4*)((const char*)yb.ts4 + zb);
    yb.tbox = (const float*)((const char*)yb.tbox + zb);
    epi.shift(z);
    if (bx < blocksA) nn_l1_block_pruned<NBT, PPL, EngineEpi, true, false>(A, na, 4, yb, 0, epi, bx, epi.stopped, B, 4);
    else if constexpr (P1) {
        pb.ts4 = (const float4*)((const char*)pb.ts4 + zb);
        pb.tbox = (const float*)((const char*)pb.tbox + zb);
        pb.nblk_dev = (const int*)((const char*)pb.nblk_dev + zb);
        nn_l1_block_pruned<NBP, PPL, EngineEpi, true, true>(B, nb, 4, pb, 1, epi, bx - blocksA, epi.stopped, A, 4);
    } else nn_l1_block<4, int, EngineEpi>(A, na, 4, B, nb, 4, nullptr, nullptr, nullptr, nullptr, blocksA, epi, bx);
}

// Round 5: the same launch with sixteen queries per wave (nn_l1_rows): both directions take their QUERIES in slot order of their own
// block-sorted copy (ps4 / ys4: neighbours in space share a wave), 64-point blocks on both sides.
template <int NBT, int NBP>
__global__ __launch_bounds__(NN_ROWS_BLOCK) void k_nn_rows(const float* A, const float* B, int blocksA, int blocksB, EngineEpi epi, NnBlocks yb, NnBlocks pb,
                                                      size_t zstride) {
    asm volatile("" :: "s"(A), "s"(B), "s"(blocksA), "s"(blocksB), "s"(epi.sgn_x), "s"(epi.cnt4), "s"(epi.lossp_x), "s"(epi.lossp_y),
                 "s"(epi.bstride), "s"(epi.stopped), "s"(yb.ts4), "s"(yb.tbox), "s"(yb.nblk), "s"(pb.ts4), "s"(pb.tbox), "s"(pb.nblk_dev), "s"(zstride));
    const int nz = gridDim.x / (blocksA + blocksB);
    int i = blockIdx.x, z, bx;
    if (i < blocksB * nz) { z = i / blocksB; bx = blocksA + (i - z * blocksB); }
    else { i -= blocksB * nz; z = i / blocksA; bx = i - z * blocksA; }
    const size_t zb = z * zstride;
    A = (const float*)((const char*)A + zb);
    B = (const float*)((const char*)B + zb);
    yb.ts4 = (const float4*)((const char*)yb.ts4 + zb);
    yb.tbox = (const float*)((const char*)yb.tbox + zb);
    pb.ts4 = (const float4*)((const char*)pb.ts4 + zb);
    pb.tbox = (const float*)((const char*)pb.tbox + zb);
    pb.nblk_dev = (const int*)((const char*)pb.nblk_dev + zb);
    epi.shift(z);
    if (bx < blocksA) nn_l1_rows<NBT, EngineEpi, false, true>(pb.ts4, 0, pb.nblk_dev, pb.nblk, yb, 0, epi, bx, epi.stopped, B, epi.lossp_x);
    else nn_l1_rows<NBP, EngineEpi, true, false>(yb.ts4, yb.nblk, nullptr, yb.nblk, pb, 1, epi, bx - blocksA, epi.stopped, A, epi.lossp_y);
}
// ------------------------------------------------------------------------------------------ host side
// The boxes per lane of a shape's two searches are template arguments (register arrays): nbt in {1, 2, 4}, nbp in {2, 3, 4, 5, 6, 8}
// (make_dims) -- f(integral_constant<nbt>, integral_constant<nbp>).
template <typename F>
static void by_boxes(int nbt, int nbp, F f) {
    by_value<1, 2, 4>(nbt, [&](auto t) { by_value<2, 3, 4, 5, 6, 8>(nbp, [&](auto p) { f(t, p); }); });
}

void launch_nn(const Dims& D, const Slice& S, size_t bstride, int par, hipStream_t s) {
    const Ws& W = S.W;
    const int nz = S.nz;
    const EngineEpi epi{W.sgn_x, W.cnt4, W.lossp_x, W.lossp_y, bstride, &W.state[par].stopped};
    if (D.rows) {
        const NnBlocks yb{W.ys4, W.ybox, D.nyb, nullptr}, pb{W.ps4, W.pbox, D.npb, W.sb + D.K};      // (pb.nblk: the host's bound, what ps4 / lossp_x are carved for)
        const int blocksA = cdiv(64 * D.npb, NN_ROW_SLOTS), blocksB = cdiv(64 * D.nyb, NN_ROW_SLOTS);
        const dim3 grid((blocksA + blocksB) * nz);
        by_boxes(D.nbt, D.nbp, [&](auto nbt, auto nbp) {
            hipLaunchKernelGGL((k_nn_rows<decltype(nbt)::value, decltype(nbp)::value>), grid, dim3(NN_ROWS_BLOCK), 0, s, (const float*)W.pred4, (const float*)W.y4,
                               blocksA, blocksB, epi, yb, pb, bstride);
        });
    } else if (D.nyb) {
        const NnGrid g = nn_grid(D.NP, D.NT, true, true, 4);
        const NnBlocks yb{W.ys4, W.ybox, D.nyb, nullptr}, pb{W.ps4, W.pbox, 0, W.sb + D.K};
        const dim3 grid((g.blocksA + g.blocksB) * nz);
        auto go = [&](auto kern, int smem) {
            hipLaunchKernelGGL(kern, grid, dim3(NN_BLOCK), smem, s, (const float*)W.pred4, D.NP, (const float*)W.y4, D.NT,
                               g.blocksA, g.blocksB, epi, yb, pb, bstride);
        };
        by_value<1, 4>(D.ppl, [&](auto ppl) {
            by_boxes(D.nbt, D.nbp, [&](auto nbt, auto nbp) {
                constexpr int PPL = decltype(ppl)::value, NBT = decltype(nbt)::value, NBP = decltype(nbp)::value;
                // the predicted cloud outside the pruned form's limits: that direction exhaustive (nbp is 2 then: no instance per nbp)
                if constexpr (NBP == 2) if (!D.npb) { go(k_nn_plan<false, PPL, NBT, 2>, g.smem); return; }
                go(k_nn_plan<true, PPL, NBT, NBP>, 0);
            });
        });
    } else {
        launch_nn_l1<int>((const float*)W.pred4, D.NP, 4, (const float*)W.y4, D.NT, 4, nullptr, nullptr, nullptr, nullptr,
                          true, true, epi, s, nz, bstride, 4);
    }
}

}  // namespace creg
using namespace creg;

// The read-backs of the measurement builds -DCREG_NN_STATS / -DCREG_NN_WAVE_STAMPS (tests/measure/README.md).  Their __device__
// globals are defined in nn_l1.h, and this build has no relocatable device code: every unit that includes the header has a copy
// of its own.  The plan's searches run k_nn_plan / k_nn_rows, which are THIS unit's, so the read-backs stay here and read the copy
// those kernels write (not nn_l1.hip's, which the stand-alone creg_nn_l1 entries write).
#ifdef CREG_NN_STATS
extern "C" int creg_debug_nn_stats(unsigned long long* out8, int reset) {
    CREG_HIP(hipMemcpyFromSymbol(out8, HIP_SYMBOL(creg::g_nn_stats), sizeof(unsigned long long) * 8));
    if (reset) { unsigned long long z[8] = {0}; CREG_HIP(hipMemcpyToSymbol(HIP_SYMBOL(creg::g_nn_stats), z, sizeof(z))); }
    return CREG_OK;
}
#endif

#ifdef CREG_NN_WAVE_STAMPS
// out: up to `cap` records of 8 x u64 {t0, t1, t2, t3, visits, candidates, direction, block}; returns the number recorded; reset != 0 clears
extern "C" long long creg_debug_nn_waves(unsigned long long* out, long long cap, int reset) {
    static unsigned n[creg::NN_WAVE_SHARDS * 32];
    if (hipMemcpyFromSymbol(n, HIP_SYMBOL(creg::g_nn_wave_n), sizeof(n)) != hipSuccess) return -1;
    long long total = 0;
    if (out && cap > 0) {
        std::vector<creg::NnWaveRec> h((size_t)creg::NN_WAVE_CAP);
        if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(creg::g_nn_wave), sizeof(creg::NnWaveRec) * (size_t)creg::NN_WAVE_CAP) != hipSuccess) return -1;
        for (unsigned sh = 0; sh < creg::NN_WAVE_SHARDS; ++sh) {
            const unsigned m = n[32 * sh] < creg::NN_WAVE_PER ? n[32 * sh] : creg::NN_WAVE_PER;
            for (unsigned i = 0; i < m && total < cap; ++i, ++total) {
                const creg::NnWaveRec& r = h[(size_t)sh * creg::NN_WAVE_PER + i];
                unsigned long long* o = out + 8 * total;
                o[0] = r.t0; o[1] = r.t1; o[2] = r.t2; o[3] = r.t3; o[4] = (unsigned long long)r.visits; o[5] = (unsigned long long)r.cands;
                o[6] = (unsigned long long)r.dir; o[7] = (unsigned long long)r.blk;
            }
        }
    } else for (unsigned sh = 0; sh < creg::NN_WAVE_SHARDS; ++sh) total += n[32 * sh];
    if (reset) { static const unsigned z[creg::NN_WAVE_SHARDS * 32] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(creg::g_nn_wave_n), z, sizeof(z)) != hipSuccess) return -1; }
    return total;
}
#endif
