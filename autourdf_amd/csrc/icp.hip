// icp.hip -- K4, the public ICP entries: one argument check, the regime switch, the workspace sizes and the two knobs.
// The kernels live in icp_small.hip (one workgroup per cluster, the whole ICP loop in one launch) and icp_large.hip (many
// workgroups per iteration, one launch per iteration); what they share is in icp_dev.h.
#include <cstdlib>
#include "icp_dev.h"

using namespace creg;

// the regime switch (host-side sizes only): average cluster above the LDS source budget, or a frame too large for the
// LDS target table to matter
static bool icp_large_regime(int64_t n, int64_t nf, int k) { return n / (k > 0 ? k : 1) > ICP_SRC_LDS || nf > 65536; }

// one problem's workspace serves either regime
static size_t icp_ws_one(int64_t n, int64_t nf, int k) {
    const size_t a = icp_small_workspace_bytes(n, nf, k), b = icp_large_workspace_bytes(n, nf, k);
    return a > b ? a : b;
}

extern "C" size_t creg_icp_workspace_bytes(int64_t n, int64_t nf, int32_t k) {
    if (n < 1 || nf < 1 || k < 1) return 0;
    return icp_ws_one(n, nf, k);
}

extern "C" size_t creg_icp_batch_workspace_bytes(int64_t n, int64_t nf, int32_t k, int32_t batch) {
    if (n < 1 || nf < 1 || k < 1 || batch < 1) return 0;
    return icp_ws_one(n, nf, k) * (size_t)batch;
}

// The environment knobs of K4.
//   CREG_ICP_SCREEN (default 1): the float32 screen of k_icp_nn; read once per process (thread-safe static).
//   CREG_ICP_P2P_ONE_WORKGROUP=1: point-to-point problems stay in the one-workgroup kernel whatever their size -- a measurement
//     knob for tests/measure/bench_icp_p2p_regimes.py, read on every call (tests flip it inside one process).
struct IcpKnobs { int screen; bool p2p_one_workgroup; };
static IcpKnobs icp_knobs() {
    static const int screen = [] { const char* e = getenv("CREG_ICP_SCREEN"); return e ? atoi(e) != 0 : 1; }();
    const char* e = getenv("CREG_ICP_P2P_ONE_WORKGROUP");
    return {screen, e && e[0] == '1'};
}

static int icp_launch(const creg_icp_problem* pr, int batch, int64_t n, int32_t k, int64_t nf, double scale, double th,
                      int32_t max_iteration, int32_t keep_translation, void* workspace, size_t workspace_bytes,
                      hipStream_t s, const char* who) {
    CREG_REQUIRE(pr && workspace, "%s: null pointer", who);
    CREG_REQUIRE(batch >= 1 && batch <= ICP_BATCH_MAX, "%s: batch must be in 1..%d", who, ICP_BATCH_MAX);
    CREG_REQUIRE(k >= 1 && nf >= 1 && nf < (1ll << 31) && max_iteration >= 1, "%s: bad size", who);
    CREG_REQUIRE(n >= 1 && n < (1ll << 31), "%s: no source points", who);
    const size_t one = icp_ws_one(n, nf, k);
    CREG_REQUIRE(workspace_bytes >= one * (size_t)batch, "%s: workspace too small (%zu < %zu)", who, workspace_bytes,
                 one * (size_t)batch);
    for (int i = 0; i < batch; ++i) {
        const creg_icp_problem& q = pr[i];
        CREG_REQUIRE(q.local && q.seg_offsets && q.frame && q.M && q.M_out && q.world_out && q.n_iter_out,
                     "%s: null pointer in problem %d", who, i);
    }
    const IcpKnobs knobs = icp_knobs();
    if (!icp_large_regime(n, nf, k) || (pr[0].tgt_offsets && knobs.p2p_one_workgroup))
        return icp_small_launch(pr, batch, n, k, nf, scale, th, max_iteration, keep_translation, (char*)workspace, one, s);
    // clusters / frames beyond what one CU's LDS holds: many workgroups per iteration instead of one per cluster
    for (int i = 0; i < batch; ++i) {
        const int rc = icp_large_run(pr[i], n, k, nf, scale, th, max_iteration, keep_translation, knobs.screen,
                                     (char*)workspace + one * (size_t)i, s);
        if (rc) return rc;
    }
    return CREG_OK;
}

extern "C" int creg_masked_icp_f64(const double* local, const float* world, const int32_t* world_offsets, int64_t n,
                                   const int32_t* seg_offsets, int32_t k, const double* frame, int64_t nf, const double* M, double scale, double th,
                                   int32_t max_iteration, int32_t keep_translation, double* M_out, double* world_out,
                                   int32_t* n_iter_out, void* workspace, size_t workspace_bytes, creg_stream_t stream) {
    const creg_icp_problem p{local, world, seg_offsets, frame, M, M_out, world_out, n_iter_out, nullptr, world_offsets};
    return icp_launch(&p, 1, n, k, nf, scale, th, max_iteration, keep_translation, workspace, workspace_bytes,
                      (hipStream_t)stream, "creg_masked_icp_f64");
}

extern "C" int creg_masked_icp_batch_f64(const creg_icp_problem* problems, int32_t batch, int64_t n, int32_t k, int64_t nf,
                                         double scale, double th, int32_t max_iteration, int32_t keep_translation,
                                         void* workspace, size_t workspace_bytes, creg_stream_t stream) {
    return icp_launch(problems, batch, n, k, nf, scale, th, max_iteration, keep_translation,
                      workspace, workspace_bytes, (hipStream_t)stream, "creg_masked_icp_batch_f64");
}

extern "C" int creg_icp_p2p_f64(const double* src, int64_t n_src, const int32_t* src_offsets, const double* tgt,
                                int64_t n_tgt, const int32_t* tgt_offsets, int32_t k, const double* init, double th,
                                int32_t max_iteration, double* T_out, double* src_out, int32_t* n_iter_out,
                                void* workspace, size_t workspace_bytes, creg_stream_t stream) {
    CREG_REQUIRE(tgt_offsets, "creg_icp_p2p_f64: null pointer");
    const creg_icp_problem p{src, nullptr, src_offsets, tgt, init, T_out, src_out, n_iter_out, tgt_offsets, nullptr};
    return icp_launch(&p, 1, n_src, k, n_tgt, 1.0, th, max_iteration, 0, workspace, workspace_bytes, (hipStream_t)stream,
                      "creg_icp_p2p_f64");
}
