/*
 * creg.h -- C ABI of libcreg.so: MI355X (gfx950) kernels for AutoURDF's cluster-registration path.
 *
 * The reference (jl6017/AutoURDF) is pure Python and has no FFI layer of its own; the boundary
 * that `match()` / scripts/registration.sh exercise is the Python module surface of
 * PointCloud/{mlp_reg,cluster_icp,dq_func}.py.  Each entry point below names the
 * reference interface (file:line under /root/reference) whose arithmetic it replaces; the
 * same-named Python modules in autourdf_amd/ bind these through ctypes (autourdf_amd/_lib.py),
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - Every data pointer is a DEVICE pointer on the current HIP device unless marked HOST.
 *   - Row-major, xyz interleaved (N,3) exactly as the reference stores clouds (mlp_reg.py:296).
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *     All work is enqueued asynchronously on it; nothing synchronises unless documented.
 *   - The library never allocates caller-visible memory and keeps no pointer after return,
 *     except inside an explicit plan object (creg_train_plan_*), which owns only the workspace
 *     the caller handed it.
 *   - Return 0 on success, a negative creg_status otherwise; creg_last_error() gives the
 *     thread-local message.  No exception crosses the boundary.
 *   - Quaternions are real-first (w,x,y,z); dual quaternions are [real | dual] (8 floats).
 */
#ifndef CREG_H
#define CREG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* creg_stream_t;

enum creg_status {
    CREG_OK = 0,
    CREG_EINVAL = -1,       /* bad argument (null pointer, negative size, unsupported option) */
    CREG_EHIP = -2,         /* a HIP runtime call failed */
    CREG_ENOTCONVERGED = -3,
    CREG_EARCH = -4         /* current device is not gfx950 */
};

int creg_version(void);                 /* 10000*major + 100*minor + patch */
const char* creg_last_error(void);
/* 0 when the current device is a gfx950 part; CREG_EARCH / CREG_EHIP otherwise. */
int creg_device_check(void);

/* ------------------------------------------------------------------------------------------
 * K1  L1 nearest neighbour (K=1), both directions of the Chamfer term.
 * Replaces pytorch3d knn_points as reached by chamfer_distance(pred, y, norm=1) at
 * mlp_reg.py:96 (and Sim/evaluation.py:81).  d = (|dx|+|dy|)+|dz| in fp32, FIRST minimum wins.
 * x (nx,3), y (ny,3) fp32.  dx (nx) / ix (nx): distance / index of the nearest y for every x;
 * dy (ny) / iy (ny): the same for every y among x.  Either direction may be skipped by passing
 * NULL for both of its outputs.  nx, ny >= 1. */
int creg_nn_l1_bidir_f32(const float* x, int64_t nx, const float* y, int64_t ny,
                         float* dx, int64_t* ix, float* dy, int64_t* iy, creg_stream_t stream);

/* Backward of  gx_scale * sum_i |x_i - y[ix_i]|_1 + gy_scale * sum_j |y_j - x[iy_j]|_1  w.r.t. x
 * with pytorch3d's sign rule (p1 > p2 ? +1 : -1).  grad_x (nx,3) is overwritten.
 * `scratch` must hold creg_nn_l1_bwd_scratch_bytes(nx) bytes. */
size_t creg_nn_l1_bwd_scratch_bytes(int64_t nx);
int creg_nn_l1_bwd_f32(const float* x, int64_t nx, const float* y, int64_t ny,
                       const int64_t* ix, const int64_t* iy, float gx_scale, float gy_scale,
                       float* grad_x, void* scratch, creg_stream_t stream);

/* mean_i dx_i + mean_j dy_j  -> *loss (one float, device).  Replaces the reduction half of
 * chamfer_distance (point_reduction = batch_reduction = "mean", batch 1). */
int creg_chamfer_l1_reduce_f32(const float* dx, int64_t nx, const float* dy, int64_t ny,
                               float* loss, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K3  per-cluster rigid transform.  Replaces calculate_pc (mlp_reg.py:155-170):
 * out[i] = R_k pts[i] + t_k for i in [seg_offsets[k], seg_offsets[k+1]), n = seg_offsets[k_last+1].
 * pts/out (n,3) fp32, M (k,4,4) fp32 row-major, seg_offsets (k+1) int32 DEVICE. */
int creg_cluster_transform_f32(const float* pts, int64_t n, const int32_t* seg_offsets, int32_t k,
                               const float* M, float* out, creg_stream_t stream);
/* grad_M (k,4,4): rows 0..2 get [sum g (x) p | sum g], row 3 is zero. */
int creg_cluster_transform_bwd_f32(const float* pts, const int32_t* seg_offsets, int32_t k,
                                   const float* grad_out, float* grad_M, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K2  Lloyd k-means, fp64, 3-D.  Replaces sklearn.cluster.k_means(X, init=<array>, n_init=1)
 * as called by resample_cluster (mlp_reg.py:204) and Segments.k_means_cluster
 * (cluster_icp.py:67, after k-means++ seeding on the host).
 *   distance  d = fma(x2,b2, fma(x1,b1, fma(x0,b0, |c|^2))),  b = -2c   (first minimum wins)
 * X (n,3) fp64 is read only (centring happens on an internal copy), init (k,3) fp64.
 * n >= k is required, as by sklearn ("n_samples=.. should be >= n_clusters=.."): the three Lloyd entry points return an error
 * before any launch otherwise (the relocation of empty clusters would run out of points to take).
 * Outputs: centers (k,3) fp64, labels (n) int32, inertia (1) fp64, n_iter (1) int32 -- device.
 * use_mfma != 0 selects the v_mfma_f64_16x16x4_f64 assignment kernel: every centre for every point, in the caller's order,
 * one launch per Lloyd iteration (E-step, exact incremental M-step sums, M-step tail; the convergence test runs on the
 * device and later launches return at once; the host enqueues 32 launches at a time and synchronises the stream in between
 * to read the `done` word).
 * use_mfma == 0 (the default of the drop-ins): the E-step runs over a spatially sorted copy of the frame and evaluates, per
 * workgroup and per wave, only the centres that can be nearest inside the bounding box of its points, and a persistent
 * kernel iterates inside one launch (the host synchronises once per run of iterations between two empty-cluster
 * relocations; when the device cannot hold the kernel's grid at once, one launch per iteration as above).  Both forms return
 * identical labels, centres, inertia and iteration counts. */
size_t creg_kmeans_workspace_bytes(int64_t n, int32_t k);
int creg_kmeans_lloyd_f64(const double* X, int64_t n, const double* init, int32_t k,
                          int32_t max_iter, double tol_rel, int32_t use_mfma,
                          double* centers, int32_t* labels, double* inertia, int32_t* n_iter,
                          void* workspace, size_t workspace_bytes, creg_stream_t stream);
/* The same k_means() for `batch` (<= 16) independent frames of identical size in ONE launch, one
 * workgroup per frame, centres and labels resident in LDS (n <= 16384, k <= 128; the centred frame too up to 5120 points, read from
 * L2 above that), fully asynchronous (no host
 * synchronisation at all).  Bit-identical to creg_kmeans_lloyd_f64.  X, init, centers, labels, inertia,
 * n_iter are HOST arrays of `batch` device pointers. */
size_t creg_kmeans_batch_workspace_bytes(int64_t n, int32_t k, int32_t batch);
int creg_kmeans_lloyd_batch_f64(const double* const* X, int64_t n, const double* const* init, int32_t k,
                                int32_t batch, int32_t max_iter, double tol_rel, double* const* centers,
                                int32_t* const* labels, double* const* inertia, int32_t* const* n_iter,
                                void* workspace, size_t workspace_bytes, creg_stream_t stream);
/* E-step only: labels[i] = argmin_k d(X_i, C_k) (no centring).  Asynchronous. */
int creg_kmeans_assign_f64(const double* X, int64_t n, const double* C, int32_t k,
                           int32_t use_mfma, int32_t* labels, creg_stream_t stream);

/* Stable grouping of points by label + change of frame, fp64.  Replaces the per-cluster mask /
 * inv(M_k) . [p;1] loop of resample_cluster (mlp_reg.py:208-217) and Segments.k_means_cluster
 * (cluster_icp.py:86-99).  M (k,4,4) fp64 local->world; out_local (n,3) holds the clusters
 * back to back in label order, each keeping the original point order; seg_offsets (k+1) int32.
 * m_is_inverse == 0: M is inverted in the kernel in fp64 (Gauss-Jordan, partial pivoting).
 * m_is_inverse != 0: M already holds inv(M_k) -- the drop-in resample_cluster inverts each pose on the host with
 * np.linalg.inv IN THE POSE'S OWN DTYPE exactly as mlp_reg.py:211 does (float32 on the default path: LAPACK sgesv,
 * whose rounding is BLAS-build specific and is not reproduced on the device), so cluster/NNNN.npz matches the
 * reference to the rounding of one 4-term fp64 dot product.  out = fma(I2,z, fma(I1,y, I0*x)) + I3 per row. */
int creg_group_to_local_f64(const double* X, int64_t n, const int32_t* labels, int32_t k,
                            const double* M, int32_t m_is_inverse, double* out_local, int32_t* seg_offsets,
                            creg_stream_t stream);
/* The same for `batch` (<= 16) frames of identical n and k in one pair of launches; X, labels, M, out_local and
 * seg_offsets are HOST arrays of `batch` device pointers.  Identical results to separate calls. */
int creg_group_to_local_batch_f64(const double* const* X, int64_t n, const int32_t* const* labels, int32_t k,
                                  const double* const* M, int32_t m_is_inverse, int32_t batch,
                                  double* const* out_local, int32_t* const* seg_offsets, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * N1  farthest-point down-sampling, fp64.  Replaces open3d farthest_point_down_sample as used by
 * Segments._load_pc (cluster_icp.py:43): start at point 0, repeatedly select the point farthest
 * (squared L2) from the selected set, first maximum wins.  sel (m) int64 indices in selection order.
 * scratch: creg_fps_scratch_bytes(n) bytes. */
size_t creg_fps_scratch_bytes(int64_t n);
int creg_fps_f64(const double* X, int64_t n, int64_t m, int64_t* sel, void* scratch, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K5  SE(3) <-> dual quaternion.  Replace transform_to_dualquat (dq_func.py:100-124) and
 * dualquat_to_transform (dq_func.py:170-186) incl. the pytorch3d matrix_to_quaternion /
 * quaternion_to_matrix they call.  M (k,4,4), dq (k,8) fp32.  The *_bwd forms give the vector-
 * Jacobian products used when these sit inside autograd (mlp_reg.py:78-84). */
int creg_se3_to_dq_f32(const float* M, int32_t k, float* dq, creg_stream_t stream);
int creg_dq_to_se3_f32(const float* dq, int32_t k, float* M, creg_stream_t stream);
int creg_dq_to_se3_bwd_f32(const float* dq, const float* grad_M, int32_t k, float* grad_dq,
                           creg_stream_t stream);
/* Remaining dq_func.py algebra on (k,8)/(k,4) rows (dq_func.py:29,47,126,148,188,213,238). */
int creg_dq_multiply_f32(const float* a, const float* b, int32_t k, float* out, creg_stream_t stream);
int creg_dq_invert_f32(const float* dq, int32_t k, float* out, creg_stream_t stream);
int creg_dq_to_quat_trans_f32(const float* dq, int32_t k, float* q, float* t, creg_stream_t stream);
int creg_quat_trans_to_dq_f32(const float* q, const float* t, int32_t k, float* dq, creg_stream_t stream);
/* pytorch3d.transforms rows used on the path (mlp_reg.py:65,68). */
int creg_matrix_to_quat_f32(const float* R, int32_t k, float* q, creg_stream_t stream);   /* R (k,3,3) */
int creg_quat_to_matrix_f32(const float* q, int32_t k, float* R, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K4  masked point-to-point ICP per cluster, fp64.  Replaces masked_icp (cluster_icp.py:118-191)
 * including open3d registration_icp (TransformationEstimationPointToPoint, max_iteration,
 * relative_fitness = relative_rmse = 1e-6).
 * local (n,3) fp64 clusters back to back (the ICP sources, n = seg_offsets[k] points in total), world fp32
 * predicted clusters back to back (only their boxes are used: cluster_icp.py:133-135), frame (nf,3) fp64 target,
 * M (k,4,4) fp64 initial poses.  world_offsets (k+1, DEVICE) are the segment offsets of `world`; NULL = the same
 * as seg_offsets.  They differ in match()'s --mlp_icp branch: `clusters_local` is the frame-0 segmentation for the
 * whole sequence (mlp_reg.py:248, never reassigned), `clusters_world` the trained clouds of the current, re-sampled
 * one (mlp_reg.py:301-306,325), so cluster i has another point count in the two lists from frame 2 on.
 * M_out (k,4,4) fp64, world_out (n,3) fp64 = M_out applied to local.  keep_translation mirrors `ori`.
 * The nearest target of a source point is found exactly (the exhaustive scan's result, lowest frame index among equidistant
 * candidates) over binned lists pruned by the distance to the previous iteration's match.
 * Two regimes, same algorithm: clusters a CU can hold (<= 1024 points on average, frames <= 65536 points) run the whole
 * loop in ONE asynchronous launch; larger ones (BASELINE configs[4]: 2048-point clusters, 262144-point frames) run it
 * one launch per iteration over many workgroups: the host enqueues batches of 16 launches and reads the number of clusters
 * (and source chunks) still iterating through pinned memory ONE BATCH BEHIND the device (round 4: no stream synchronisation in
 * the loop; the call returns when the counters it has read say "converged", with at most one surplus batch of empty launches
 * and the final copy-out still in the queue -- outputs are ready when the stream is).  The results of the two regimes agree to
 * rounding (different summation trees), not bit for bit.
 * workspace: creg_icp_workspace_bytes(n, nf, k). */
size_t creg_icp_workspace_bytes(int64_t n, int64_t nf, int32_t k);
int creg_masked_icp_f64(const double* local, const float* world, const int32_t* world_offsets, int64_t n,
                        const int32_t* seg_offsets, int32_t k, const double* frame, int64_t nf, const double* M,
                        double scale, double th, int32_t max_iteration, int32_t keep_translation,
                        double* M_out, double* world_out, int32_t* n_iter_out,
                        void* workspace, size_t workspace_bytes, creg_stream_t stream);

/* The same for `batch` (<= 16) independent problems of identical n, nf and k (the frames of several
 * sequences) in ONE launch: grid (k, batch).  Results are those of `batch` separate calls, bit for bit.
 * workspace: creg_icp_batch_workspace_bytes(n, nf, k, batch). */
typedef struct creg_icp_problem {
    const double* local; const float* world; const int32_t* seg_offsets; const double* frame; const double* M;
    double* M_out; double* world_out; int32_t* n_iter_out;
    const int32_t* tgt_offsets;   /* NULL: masked mode above.  Non-NULL (k+1 offsets into `frame`): point-to-point
                                     mode, cluster i registers to frame[tgt_offsets[i] .. tgt_offsets[i+1]) unmasked,
                                     `world` is ignored and nf is the total number of target points */
    const int32_t* world_offsets; /* masked mode: (k+1) segment offsets of `world`; NULL = seg_offsets */
    /* masked mode with world == NULL: the mask boxes are those of the clusters in their CURRENT pose, i.e. of
       float32(M) applied to float32(local) exactly as creg_cluster_transform_f32 evaluates it -- the caller
       saves that launch and the two casts */
} creg_icp_problem;
size_t creg_icp_batch_workspace_bytes(int64_t n, int64_t nf, int32_t k, int32_t batch);
int creg_masked_icp_batch_f64(const creg_icp_problem* problems, int32_t batch, int64_t n, int32_t k, int64_t nf,
                              double scale, double th, int32_t max_iteration, int32_t keep_translation,
                              void* workspace, size_t workspace_bytes, creg_stream_t stream);

/* Step 1 of masked_icp on its own (cluster_icp.py:133-146): per cluster the float32 axis-aligned box of its predicted
 * world points scaled about its centre, and the indices of the frame points strictly inside it, ascending.
 * world fp32 clusters back to back with offsets world_offsets (k+1), frame (nf,3) fp64.  mask_idx (k, nf) int32: row c
 * holds mask_count[c] indices; boxes (k,6) fp32 [lo xyz | hi xyz] or NULL.  The same kernel as the large-cluster regime
 * of creg_masked_icp_f64 runs first. */
int creg_aabb_mask_f64(const float* world, const int32_t* world_offsets, int32_t k, const double* frame, int64_t nf,
                       double scale, int32_t* mask_idx, int32_t* mask_count, float* boxes, creg_stream_t stream);

/* The closed-form fit alone (SURVEY 8(b) / north star "per-cluster weighted SVD / least-squares SE(3) pose fits"): for every
 * segment [offsets[c], offsets[c+1]) of the PAIRED points src[i] <-> dst[i] ((n,3) fp64 each) the rigid T_out[c] (4x4 fp64)
 * minimising sum_i w_i |T src_i - dst_i|^2 (weights (n) fp64 >= 0, or NULL for 1) -- what open3d's
 * TransformationEstimationPointToPoint::ComputeTransformation (Eigen::umeyama without scaling, reflection fix) returns for
 * the correspondences of one ICP iteration (cluster_icp.py:157 through registration_icp).  A segment with no weight at all
 * gets the identity.  Horn's quaternion form: always a proper rotation; where the optimum is not unique (collinear or fewer
 * than three distinct pairs) it returns one of the minimisers. */
int creg_kabsch_f64(const double* src, const double* dst, const double* weights, int64_t n, const int32_t* offsets,
                    int32_t k, double* T_out, creg_stream_t stream);

/* N3  plain point-to-point ICP of k independent (source, target) cloud pairs in one launch: the
 * registration_icp(source, target, threshold, init, TransformationEstimationPointToPoint,
 * ICPConvergenceCriteria(max_iteration)) calls of link.refine_links_clusters (link.py:85-127, th = 1,
 * init = I, per link and time step) and Sim/evaluation.py:358-362 (th = 0.01).  Same kernel, iteration and
 * stopping rule as K4 without the box mask.  src (n_src,3) / tgt (n_tgt,3) fp64 segments back to back,
 * init and T_out (k,4,4) fp64, src_out = T_out applied to src.  Several time steps per launch:
 * creg_masked_icp_batch_f64 with tgt_offsets set.  workspace: creg_icp_workspace_bytes(n_src, n_tgt, k). */
int creg_icp_p2p_f64(const double* src, int64_t n_src, const int32_t* src_offsets, const double* tgt, int64_t n_tgt,
                     const int32_t* tgt_offsets, int32_t k, const double* init, double th, int32_t max_iteration,
                     double* T_out, double* src_out, int32_t* n_iter_out,
                     void* workspace, size_t workspace_bytes, creg_stream_t stream);

/* Measurement hook of the many-workgroup ICP regime (the frame of BASELINE configs[4]; bench.py's roofline of that leg): work counters
 * of the search kernel k_icp_nn, always on (wave-uniform tallies, one atomic per counter and wave), and -- while `timing` is set -- a
 * pair of HIP events around every k_icp_nn launch on the launch stream (the call then ends with a stream synchronisation).
 * out8 (HOST, 8 doubles, may be NULL): [0] waves that searched, [1] float32 screen trips (a trip = 8 staged targets x 64 lanes = 512
 * pair evaluations), [2] trips that went on to the fp64 evaluation, [3] source-iterations (live sources summed over launches),
 * [4] tie rescans, [5] summed k_icp_nn launch time in microseconds, [6] launches timed, [7] 0.  reset != 0: zero all of it afterwards.
 * timing: 1 / 0 switches the event bracketing on / off, < 0 leaves it.  Synchronises the device (hipMemcpyFromSymbol).
 * The hook is for ONE host thread and the CURRENT device: the timing switch and its two tallies are plain process-wide host state
 * (no lock, no atomics), the work counters are those of the device that is current when it is called. */
int creg_icp_nn_counters(double* out8, int32_t reset, int32_t timing);

/* ------------------------------------------------------------------------------------------
 * N2  pose-sequence distance maps, fp64: the consumer of match()'s matrix/NNNN.npy files.  Replaces the
 * Python loops of CoordMap.coord_dist_map (coord_map.py:230-307; roma rotmat_to_rotvec,
 * utils.rotvec_geodesic_distance and rotmat_geodesic_distance inside) and load_matrix's
 * pose -> xyz + quaternion step (coord_map.py:204-219).
 * M (T,K,4,4) fp64 poses.  diff != 0: T-1 maps built from step-to-step motion differences and the
 * row-distance step (:250-281); diff == 0: T maps of pose distances (:283-301).
 * d_map (K,K,T') fp64 laid out like np.stack(..., axis=2); sum_map (K,K) = sum_t |d_map| (:304-305).
 * A NaN in a rotation block stays NaN (the clamp in front of acos keeps it, like torch.clamp): row and column k
 * of that step for diff == 0, the two steps that use the pose for diff != 0, and sum_map wherever a step is NaN.
 * bounding_box = CoordMap.bounding_box (diagonal of the raw clouds' AABB, :153-173).
 * coords (n,7) = [x, y, z, qw, qx, qy, qz] with pytorch3d's matrix_to_quaternion in fp64. */
size_t creg_coord_dist_map_workspace_bytes(int32_t T, int32_t K);
int creg_coord_dist_map_f64(const double* M, int32_t T, int32_t K, double bounding_box, int32_t diff,
                            double* d_map, double* sum_map, void* workspace, size_t workspace_bytes,
                            creg_stream_t stream);
int creg_pose_coords_f64(const double* M, int64_t n, double* coords, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * N4  the graph half of the URDF stage (coord_map.py:70-128, :334-349), fp64, one workgroup per call.
 *
 * creg_link_sweep_f64: link discovery for every candidate link count nl in [nl_lo, nl_hi) in one launch --
 * coord_clustering(K, d_map, nl) for each nl and silhouette_score_method's choice.
 *   d_map (K,K) fp64, the normalised sum map; only its strict upper triangle defines the graph ({i<j : d[i][j] < t}),
 *     the full rows feed the silhouette.  2 <= K <= 256 (kept in LDS up to K = 128, read from global above);
 *     1 <= nl_lo < nl_hi <= K + 1.  Entries must be finite (the caller checks).
 *   thresholds (n) : the float64 lattice point t_k (t_0 = 1, t_{k+1} = fl(t_k - 1e-4) by repeated subtraction) at which
 *     the reference's loop first sees >= nl components -- the value BEFORE its decrement / print.  n = nl_hi - nl_lo.
 *   labels (n,K) int32 : component of every node at that threshold, components numbered by their smallest node
 *     (networkx.connected_components order);  n_comp (n) int32 : the component count.
 *   scores (n) : sklearn silhouette_score(d_map, labels, metric="precomputed") (row sums in index order per cluster,
 *     intra / (n_c - 1), minimum inter-cluster mean, singletons 0, NaN 0, numpy's pairwise mean); NaN where the
 *     label count is outside [2, K-1].  A partition always gets the same bits, whichever nl produced it.
 *   best (1) int32 : index of the first maximum score (np.argmax), or -1 when some nl had a label count outside
 *     [2, K-1] (sklearn raises ValueError there; the Python layer raises it).
 * The components come from one Prim MST of the upper triangle (any MST gives the same components).
 *
 * creg_coord_mst_f64: CoordMap.coord_mst.  coords (T,K,7) fp64 ([xyz, quaternion], load_matrix's layout); the xyz are
 *   summed over T and Prim runs on their Euclidean distance matrix from node 0.  edges (K-1,2) int32 = (tree node, new
 *   node) and weights (K-1) fp64, in the order Prim attaches them.  2 <= K <= 256.
 *   Tie rule: among equal keys the smallest node index is attached first, and a node's key is replaced only by a
 *   strictly smaller weight.  With distinct weights the MST is unique and equals networkx's Kruskal result; the
 *   Python layer restores networkx's edge order (weights ascending, ties row-major). */
int creg_link_sweep_f64(const double* d_map, int32_t K, int32_t nl_lo, int32_t nl_hi, int32_t* labels,
                        int32_t* n_comp, double* thresholds, double* scores, int32_t* best, creg_stream_t stream);
int creg_coord_mst_f64(const double* coords, int32_t T, int32_t K, int32_t* edges, double* weights,
                       creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * N4  the geometric half of the URDF stage (compute_joints.py:10-268, coord_map.py:443-502), fp64.
 *
 * Links are passed as a flat cluster list link_clusters (n_link_clusters int32) plus link_offsets (L+1 int32): link l is
 * link_clusters[link_offsets[l] .. link_offsets[l+1]), in the iteration order of the reference's cluster_idx set (the
 * kernels never sort it; every sum runs in that order).  Every link holds >= 1 cluster, every index is in [0, K), K <= 256.
 *
 * creg_joint_axes_f64: estimate_joint_axes_from_tree for every joint in one launch (one workgroup per joint).
 *   coords (S,T,K,7) fp64 = load_matrix's [xyz, wxyz] of S sequences.  joints (J,2) int32 = (parent link, child link) as
 *   indices into link_offsets, in the order the reference visits them.  Samples of a joint: sequence-major, then phase
 *   a in [0, interval), then step k >= 1 of range(start_step + a, start_step + num_steps, interval); sample (s, a, k)
 *   relates coords[s, i - interval] and coords[s, i], i = start_step + a + k * interval.  start_step + num_steps <= T
 *   (the host raises IndexError first); creg_joint_axes_samples(S, num_steps, interval) = NS <= 4096 samples per joint.
 *   Per sample (J,NS): sample_axis (3) unit direction, sample_angle in [0, pi], sample_point (3) the canonical point of the
 *   axis (init_position, compute_joints.py:68-77), sample_usable int32.  Each sample's angle is >= 0 (axis and angle as
 *   one pair (d, theta); the reference may return (-d, -theta)).  A sample is usable iff theta >= 2e-4 rad and the
 *   outputs are finite; an unusable sample has NaN axis and point.  A link whose cluster poses at a step hold a NaN or an
 *   Inf -- in a position or in a quaternion, whose average is then NaN -- makes the samples that touch that step unusable.
 *   Per joint: local_axis (J,3) = the principal axis, local_pos (J,4) = optimize_joint_axis's principal_pos (homogeneous),
 *   global_pos (J,3), global_axis (J,3) = R_child(first pose) @ local_axis, count (J) int32 usable samples,
 *   first_pose (J,2,7) or NULL = get_cluster_pose_mean of the parent and the child at sequence 0, step start_step
 *   ([xyz, wxyz]; the average quaternion's sign is the eigen solver's).
 *   SIGN CONVENTION: local_axis points so that the joint's first usable sample has a positive angle (the reference's
 *   principal axis follows the sign np.linalg.eig gives its first axis: it equals this one up to one sign per joint).
 *   A joint with count 0 gets NaN outputs.  The child's first-pose matrix is rounded to float32 as the reference's
 *   xyzquant2matrix_torch rounds it, and inverted as a general 4x4 in fp64.
 *
 * creg_link_clouds_f64: CoordMap.cluster_to_link for T frames and L links: workgroups over (frame, link) x slices of
 *   1024 output rows; max_link_rows (HOST) = the largest out_offsets[i+1] - out_offsets[i] sizes the slices (a smaller
 *   value costs speed, never rows: a workgroup strides over the slices of its (frame, link)).
 *   coords (T,K,7) fp64, matrices (T,K,4,4) fp64 the cluster poses.  points (n_points,3) fp64: every frame's local
 *   cluster points packed frame-major, cluster k of frame t at point_offsets[t*K + k .. t*K + k + 1) (T*K + 1 int64).
 *   out_offsets (T*L + 1 int64): link l of frame t fills rows out_offsets[t*L + l ..) of clouds_wf / clouds_lf
 *   (n_out,3) fp64, its clusters concatenated in set order (the host sizes them; nothing is written past n_out).
 *   link_matrices (T,L,4,4) float32 = quaternion_to_matrix of the fp64 mean cluster coords, rounded to float32.
 *   A link whose cluster quaternions sum to exactly zero (q and -q) divides by |q|^2 = 0 as the reference does: the
 *   rotation block of its link_matrices is NaN (translation and last row stay finite) and its clouds_lf rows are NaN;
 *   its clouds_wf and mean_matrices, and every other (frame, link) of the launch, are unaffected.
 *   mean_matrices (T,L,4,4) float32 or NULL = create_urdf's link transform: the float32 mean (summed in set order) of the
 *   clusters' float32 matrices.  clouds_wf = local @ R_k^T + t_k; clouds_lf = clouds_wf moved by the fp64 inverse of the
 *   float32 link matrix.  Traffic: 24 B read and 48 B written per point. */
int creg_joint_axes_samples(int32_t S, int32_t num_steps, int32_t interval);
int creg_joint_axes_f64(const double* coords, int32_t S, int32_t T, int32_t K, const int32_t* link_clusters,
                        const int32_t* link_offsets, int32_t n_link_clusters, const int32_t* joints, int32_t J,
                        int32_t start_step, int32_t num_steps, int32_t interval, double* sample_axis, double* sample_angle,
                        double* sample_point, int32_t* sample_usable, double* local_axis, double* local_pos,
                        double* global_pos, double* global_axis, int32_t* count, double* first_pose,
                        creg_stream_t stream);
int creg_link_clouds_f64(const double* coords, const double* matrices, int32_t T, int32_t K, const int32_t* link_clusters,
                         const int32_t* link_offsets, int32_t n_link_clusters, int32_t L, const double* points,
                         const int64_t* point_offsets, int64_t n_points, const int64_t* out_offsets, int64_t n_out,
                         int64_t max_link_rows, float* link_matrices, float* mean_matrices, double* clouds_wf,
                         double* clouds_lf, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Joint motion: where every joint stood at every step, how well one revolute axis explains it, and how a replayed
 * URDF compares with the registration (this project's own; the reference writes a placeholder limit).  fp64, no
 * floating-point atomics: two runs give the same bits, and a joint gives the same bits alone and among others.
 * R[r][c] below is a rotation's row r, column c; a "rigid inverse" of [R t] is [R^T, -R^T t] with R taken as orthonormal.
 * For a rotation matrix R:  v(R) = ((R21 - R12)/2, (R02 - R20)/2, (R10 - R01)/2),  c(R) = (((R00 + R11) + R22) - 1)/2,
 * so that v = sin(angle) axis and c = cos(angle).
 *
 * creg_link_poses_f64: one thread per (s, t, l).  coords (S,T,K,7) fp64 = [xyz, wxyz]; links as for creg_joint_axes_f64
 *   (link_clusters / link_offsets, L links).  link_T (S,T,L,4,4) fp64, row-major: exactly the mean pose
 *   creg_joint_axes_f64 computes for the link at that step -- the mean xyz summed in list order and divided by the list's
 *   length, the top eigenvector (cyclic Jacobi) of (1/n) sum q q^T summed in list order, its quaternion_to_matrix --
 *   written as [R t; 0 0 0 1] without rounding to float32.  A cluster index outside [0, K) is skipped (the host rejects
 *   it first).  K <= 256, S*T*L < 2^31.
 *
 * creg_joint_positions_f64: link_T (S,T,L,4,4) as above.  joints (J,2) int32 = (parent link, child link).  local_axis
 *   (J,3) and local_pos (J,4) as creg_joint_axes_f64 returns them: in the child's frame, the axis taken as a unit vector,
 *   only local_pos[0..2] read.  Steps used: t = start_step + i, i in [0, num_steps); start_step + num_steps <= T,
 *   0 <= ref_seq < S, 0 <= ref_step < T (the host raises IndexError first); S <= 65535.
 *   Per joint: X(s,t) = P^-1 C (rigid inverse of the parent's link_T times the child's), X0 = X(ref_seq, ref_step),
 *   D = X0^-1 X(s,t) (rigid inverse again) = [R d].  For a revolute joint D is the rotation by the joint position about
 *   a = local_axis through p = local_pos.
 *   Per sample (J,S,num_steps):
 *     w    = atan2((v0 a0 + v1 a1) + v2 a2, c) with v = v(R), c = c(R): the wrapped position in (-pi, pi].
 *     q    = the position unwrapped per sequence along i: u(0) = w(0);  u(i) = u(i-1) + (d - 2pi * rint(d / 2pi)) with
 *            d = w(i) - w(i-1), 2pi the double 6.283185307179586, rint rounding half to even.  One thread runs the
 *            recurrence in this order.  A non-finite w(i) therefore makes u non-finite from step i to the end of ITS sequence.
 *     tilt = atan2(|v(E)|, c(E)) >= 0 for E = Rot(a, -w) R, Rot(a, x) = I + sin x [a]x + (1 - cos x) [a]x [a]x: the angle of
 *            the rotation left once the turn about the axis is taken out.
 *     slip = |(R p + d) - p|: a point of the axis stays put under a revolute joint.
 *   Per joint: summary (J,6) = lower = min u, upper = max u, tilt_rms = sqrt(sum tilt^2 / n_used), tilt_max, slip_rms,
 *   slip_max; where (J,5) int32 = n_used, (s, i) of the minimum, (s, i) of the maximum; ties go to the first sample in
 *   (s, i) order.  A sample whose u, tilt or slip is not finite is left out of the summary and of n_used; its per-sample
 *   outputs stay as computed.  The two sums of squares run over 256 threads, thread k taking samples k, k + 256, ... of the
 *   (s, i) order, then the wave's xor butterfly (offsets 32 .. 1), then the four waves in order: an order (S, num_steps)
 *   alone decides.  n_used = 0 (a NaN axis, a non-finite reference pose): the six figures are NaN and the four indices -1.
 *   A joint whose link index is outside [0, L) is skipped: nothing of it is read or written.  J = 0 launches nothing.
 *   Two launches (samples over (joint, sequence) workgroups, then one workgroup per joint), both latency-bound.
 *
 * creg_motion_error_f64: one thread per (pose, link).  A, B (P,L,4,4), A0, B0 (L,4,4), point (L,3), fp64.
 *   Ma = A A0^-1 and Mb = B B0^-1 (rigid inverses: R = R_X R_X0^T, t = t_X - R t_X0).  rot_err (P,L) = atan2(|v(Rr)|, c(Rr))
 *   for Rr = R_Ma^T R_Mb; pos_err (P,L) = |Ma x - Mb x| for x = point[l].  The error is free of frames: it compares how a
 *   link moved from its reference pose under two descriptions, whatever frame each one attaches to the link.  P*L < 2^31.
 *
 * creg_joint_types_f64: which kind of joint every edge is -- the companion of creg_joint_axes_f64, with its launch shape
 *   (one workgroup of 256 threads per joint, thread k taking samples k, k + 256, ...) and its samples (sequence-major,
 *   then phase, then step; NS = creg_joint_axes_samples(S, num_steps, interval) <= 4096, K <= 256).  coords, links and
 *   joints as there, plus L, the number of links (link_offsets holds L+1 entries).  turn_min (rad) and slide_min (the
 *   clouds' unit) are finite and >= 0 (the host rejects anything else).
 *   Per sample: D = X_{i-1}^-1 X_i = [R t] built exactly as creg_joint_axes_f64 builds it (the links' mean poses, X = P^-1 C
 *   by the rigid inverse, then X_{i-1}^-1 X_i by the rigid inverse), theta = atan2(|v(R)|, c(R)) with
 *   |v| = sqrt((v0 v0 + v1 v1) + v2 v2): the bits of creg_joint_axes_f64's sample_angle on the same input.  t is the
 *   translation of D, in the child's frame at step i - interval, and |t| = sqrt((t0 t0 + t1 t1) + t2 t2).
 *   Per sample (J,NS): sample_angle = theta, sample_slide (3) = t, sample_kind int32:
 *     -1  theta or a component of t is not finite
 *      1  (turn)   theta >= turn_min
 *      2  (slide)  theta < turn_min and |t| >= slide_min
 *      0  (still)  otherwise
 *   Per joint: counts (J,4) int32 = n_still, n_turn, n_slide, n_bad;  type (J) int32 in creg_urdf_fk_f64's numbering:
 *      1 (revolute) if n_turn > 0 -- with turn_min = 2e-4 exactly the joints creg_joint_axes_f64 gives count > 0 for
 *      (finite outputs granted);  else 2 (prismatic) if n_slide > 0;  else 0 (fixed) if n_still > 0;  else -1 (no finite
 *      sample, or NS = 0).
 *   slide_axis (J,3) = the unit top eigenvector (cyclic Jacobi, ties: the first largest diagonal) of sum t t^T over the
 *   slide samples, signed so that (a0 t0 + a1 t1) + a2 t2 >= 0 for the first slide sample in sample order (the convention
 *   of local_axis); NaN when n_slide = 0.  The six sums run per thread in stride order, then the wave's xor butterfly
 *   (offsets 32 .. 1), then the four waves in order.  No atomics on floating-point data: two runs give the same bits, a
 *   joint alone the bits it gives among others.
 *   global_axis (J,3) = R_child(sequence 0, step start_step) slide_axis (NaN with it);  global_pos (J,3) = the child's mean
 *   position at that pose rounded to float32, as creg_joint_axes_f64's first-pose matrix holds it.  The joint point of a
 *   prismatic or fixed joint is the child's origin: its local_pos is (0,0,0,1) by definition.
 *   A joint whose link index is outside [0, L) is skipped: nothing of it is read or written.  J = 0 launches nothing.
 *   With NS = 0 the per-sample outputs may be NULL and are not touched.  One launch, latency-bound.
 *
 * creg_joint_slides_f64: the prismatic / fixed counterpart of creg_joint_positions_f64.  link_T, joints, ref_seq, ref_step,
 *   start_step, num_steps and their bounds as there; local_axis (J,3) in the child's frame, taken as a unit vector or, for
 *   a fixed joint, as zero; there is no local_pos.  D = X0^-1 X(s,t) = [R d] as there.
 *   Per sample (J,S,num_steps):
 *     q    = (d0 a0 + d1 a1) + d2 a2: the slide along the axis; nothing is unwrapped.
 *     tilt = atan2(|v(R)|, c(R)) >= 0: the whole rotation is unexplained.
 *     slip = |d - q a|: the motion off the axis.  A fixed joint passes a = 0: q = 0 and slip = |d|.
 *   Per joint: summary (J,6) and where (J,5) by the second launch of creg_joint_positions_f64, unchanged, in its layout.
 *   A joint whose link index is outside [0, L) is skipped.  J = 0 launches nothing.  Two launches, both latency-bound. */
int creg_joint_types_f64(const double* coords, int32_t S, int32_t T, int32_t K, const int32_t* link_clusters,
                         const int32_t* link_offsets, int32_t n_link_clusters, int32_t L, const int32_t* joints, int32_t J,
                         int32_t start_step, int32_t num_steps, int32_t interval, double turn_min, double slide_min,
                         double* sample_angle, double* sample_slide, int32_t* sample_kind, int32_t* counts, int32_t* type,
                         double* slide_axis, double* global_axis, double* global_pos, creg_stream_t stream);
int creg_joint_slides_f64(const double* link_T, int32_t S, int32_t T, int32_t L, const int32_t* joints, int32_t J,
                          const double* local_axis, int32_t ref_seq, int32_t ref_step, int32_t start_step,
                          int32_t num_steps, double* q, double* tilt, double* slip, double* summary, int32_t* where,
                          creg_stream_t stream);
int creg_link_poses_f64(const double* coords, int32_t S, int32_t T, int32_t K, const int32_t* link_clusters,
                        const int32_t* link_offsets, int32_t n_link_clusters, int32_t L, double* link_T,
                        creg_stream_t stream);
int creg_joint_positions_f64(const double* link_T, int32_t S, int32_t T, int32_t L, const int32_t* joints, int32_t J,
                             const double* local_axis, const double* local_pos, int32_t ref_seq, int32_t ref_step,
                             int32_t start_step, int32_t num_steps, double* q, double* tilt, double* slip,
                             double* summary, int32_t* where, creg_stream_t stream);
int creg_motion_error_f64(const double* A, const double* A0, const double* B, const double* B0, const double* point,
                          int32_t P, int32_t L, double* rot_err, double* pos_err, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Link meshing (PointCloud/link.py:204-314, link_mesh; DESIGN N4).  The contract is this project's own, NOT pinned to
 * Open3D / PyMCubes / pymeshfix.  Every call takes all L links of one directory: points (n,3) fp64 concatenated with
 * offsets (L+1) int64, per-link outputs concatenated the same way.
 *
 * creg_statistical_outlier_f64: avg (n) = mean distance to the k' = min(nb_neighbors, n_link) nearest points of the own
 *   link (self included, exact search); per link over avg > 0: thr (L) = mean + std_ratio * sample deviation (NaN with
 *   fewer than two such points); keep (n) uint8 = avg > 0 && avg < thr.  nb_neighbors outside [1, 32]: CREG_EINVAL.
 * creg_voxel_bounds_f64: over the kept points (keep may be NULL = all): origin (L,3) = min - voxel_size / 2, dims (L,3)
 *   int32 = largest floor((p - origin) / voxel_size) + 1, n_kept (L) int64.
 * creg_voxel_layout: HOST arrays in, HOST node_offsets (L+1) out, launches nothing.  The volume of link l has dims + 2
 *   nodes per axis (one empty layer on every side), node (x,y,z) at (x * Y + y) * Z + z.  CREG_EINVAL for a link without
 *   kept points, a padded axis above 1024 nodes, or more than 2^28 nodes in total.
 * creg_voxel_fill_f64: occ (total_nodes) bytes, zeroed and filled here.
 * creg_mc_count_u8: marching cubes at level 0.5, phase 1: classifies every cell, leaves the case masks and the scanned
 *   per-node vertex / triangle prefixes in the workspace (creg_mc_workspace_bytes) and writes vert_offsets (L+1) and
 *   tri_offsets (L+1) int64 (device), which the host reads to size phase 2's outputs.
 * creg_mc_emit_i32: phase 2 on the same workspace: verts_h (V,3) int32 in half-voxel units of the unpadded grid (numbered
 *   per link by owning node in linear order, then axis), tris (F,3) int32 local to the link (cell linear order, then
 *   table order; normals point from occupied to empty).
 * creg_mesh_finish_f64: vertices (V,3) fp64 = origin + (voxel_size / 2) * v', v' = (v + sum of neighbours) / (1 + deg)
 *   with integer sums when smooth != 0 (workspace: creg_mesh_finish_workspace_bytes), v' = v otherwise; stl_records
 *   (F,4,3) float32: unit normal of the float32-rounded vertices ((0,0,0) for zero area), then the three vertices.
 * voxel_size <= 0 or non-finite: CREG_EINVAL.  A refused call launches nothing. */
int creg_statistical_outlier_f64(const double* points, int64_t n, const int64_t* offsets, int32_t L, int32_t nb_neighbors,
                                 double std_ratio, double* avg, double* thr, uint8_t* keep, creg_stream_t stream);
int creg_voxel_bounds_f64(const double* points, int64_t n, const int64_t* offsets, int32_t L, const uint8_t* keep,
                          double voxel_size, double* origin, int32_t* dims, int64_t* n_kept, creg_stream_t stream);
int creg_voxel_layout(const int32_t* dims, const int64_t* n_kept, int32_t L, int64_t* node_offsets);
int creg_voxel_fill_f64(const double* points, int64_t n, const int64_t* offsets, int32_t L, const uint8_t* keep,
                        double voxel_size, const double* origin, const int32_t* dims, const int64_t* node_offsets,
                        int64_t total_nodes, uint8_t* occ, creg_stream_t stream);
size_t creg_mc_workspace_bytes(int64_t total_nodes);
int creg_mc_count_u8(const uint8_t* occ, const int32_t* dims, const int64_t* node_offsets, int32_t L, int64_t total_nodes,
                     int64_t* vert_offsets, int64_t* tri_offsets, void* workspace, size_t workspace_bytes,
                     creg_stream_t stream);
int creg_mc_emit_i32(const int32_t* dims, const int64_t* node_offsets, int32_t L, int64_t total_nodes,
                     const int64_t* vert_offsets, int64_t V, int64_t F, int32_t* verts_h, int32_t* tris, void* workspace,
                     size_t workspace_bytes, creg_stream_t stream);
size_t creg_mesh_finish_workspace_bytes(int64_t V);
int creg_mesh_finish_f64(const int32_t* verts_h, int64_t V, const int32_t* tris, int64_t F, const int64_t* vert_offsets,
                         const int64_t* tri_offsets, int32_t L, const double* origin, double voxel_size, int32_t smooth,
                         double* vertices, float* stl_records, void* workspace, size_t workspace_bytes,
                         creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Convex collision hulls of the links (DESIGN N4): the exact convex hull of every link's lattice points, all links of a
 * call in one launch, one workgroup per link.  The contract is this project's own.
 *   inputs     pts (n,3) int32, the links concatenated (the mesher's verts_h: half-voxel units); offsets (L+1) int64 on the
 *              device and the same values in offsets_host, which this entry checks before it launches; max_abs: the largest
 *              |coordinate| if the host knows it, a negative value if it does not.
 *   build      creg_lattice_hull_i32 writes status (L) int32 and face_count (L) int32 and leaves every link's faces in the
 *              workspace (creg_lattice_hull_workspace_bytes(n, L): 24 bytes per point, 88 per face slot, 2 n + 4 L slots).
 *              The host reads face_count -- the one wait, as between creg_mc_count_u8 and creg_mc_emit_i32 -- and sizes
 *   emit       creg_lattice_hull_emit_i32 on the same workspace: triangles (F,3) int32, indices local to the link's rows of
 *              pts, link l at rows tri_offsets[l] .. tri_offsets[l+1] (device, (L+1) int64, the prefix sums of face_count),
 *              in face-slot order.  With stl_records != NULL the same launch writes (F,4,3) float32 records in the format of
 *              creg_mesh_finish_f64 without smoothing: world = origin[l] + (voxel_size / 2) * v in fp64, rounded to float32;
 *              the unit normal of the rounded vertices, (0,0,0) if they span no area.  The host only packs bytes.
 * A link of status CREG_HULL_OK:
 *   convex     the triangles are a closed, consistently oriented surface of genus 0: every directed edge occurs exactly once
 *              and so does its reverse, V - E + F = 2, normals point outward, no triangle has zero area, and for every
 *              face (a,b,c) and every point p of the link det(b-a, c-a, p-a) <= 0, exactly.
 *   exact      every predicate is an integer determinant in int64; no floating point decides anything and there is no
 *              tolerance.  |coordinate| <= 16383, so a component of (b-a) x (c-a) is below 2^31 and a determinant below
 *              6 * 2^45.  max_abs > 16383 is CREG_EINVAL before any launch; a link that holds such a coordinate
 *              when max_abs < 0 gets CREG_HULL_ERANGE.
 *   vertices   the vertices used are input points (indices, so trivially) and include every extreme point of the link's
 *              set.  A point interior to a hull facet or edge is never inserted as an apex (only det > 0 is outside) but may
 *              be a vertex if it was extreme when inserted; coplanar facets are triangulated as the insertion order left them.
 *   ties       always to the smallest point index: the seed is the lexicographically smallest point, the farthest from it
 *              (squared distance), the farthest from that line (squared cross product, in uint64), the farthest from that
 *              plane (|det|); a round's apex is the point of the lowest face slot that has points above it with the
 *              largest determinant there; a face is visible from the apex when its determinant is >= 0.
 *   same bits  no atomics of any kind; every list is kept in a fixed order.  Two runs give the same bits, and a link alone in
 *              a call gives the same bits as among others.  Nothing outside the outputs and the first
 *              creg_lattice_hull_workspace_bytes(n, L) bytes of the workspace is written.
 *   bounded    a round removes its apex from the list of outside points, so a link of n_l points runs at most n_l rounds;
 *              the live faces never exceed 2 n_l - 4 and a round needs at most 2 fresh slots, so 2 n_l + 4 slots suffice.
 *              Each bound is checked: CREG_HULL_EBOUND, CREG_HULL_EWORKSPACE, and CREG_HULL_ETOPOLOGY when a horizon is
 *              not one closed cycle.  None of the three can occur unless the kernel is wrong; no loop waits for another
 *              thread or workgroup.
 * Any other status: face_count 0 and no triangle; every other link of the call is unaffected.  CREG_HULL_EFEW: fewer than
 * 4 points; CREG_HULL_EIDENTICAL / ECOLLINEAR / ECOPLANAR: the points span no volume (duplicated points are otherwise
 * fine); CREG_HULL_EOFFSETS: offsets[l] .. offsets[l+1] is no range inside 0 .. n (only if the device's offsets differ from
 * offsets_host).
 * CREG_EINVAL, nothing launched: n < 0 or > 2^28, L < 1 or > 2^20, a null pointer, offsets_host not non-decreasing from 0 to
 * n, max_abs > 16383, a workspace that is too small; in emit also n_tri < 0 or > 2 n, and stl_records without an origin or
 * with a voxel_size that is not positive and finite. */
enum creg_hull_status {
    CREG_HULL_OK = 0,
    CREG_HULL_EFEW = 1,
    CREG_HULL_EIDENTICAL = 2,
    CREG_HULL_ECOLLINEAR = 3,
    CREG_HULL_ECOPLANAR = 4,
    CREG_HULL_ERANGE = 5,
    CREG_HULL_EOFFSETS = 6,
    CREG_HULL_EWORKSPACE = 7,
    CREG_HULL_EBOUND = 8,
    CREG_HULL_ETOPOLOGY = 9
};
size_t creg_lattice_hull_workspace_bytes(int64_t n, int32_t n_links);
int creg_lattice_hull_i32(const int32_t* pts, int64_t n, const int64_t* offsets, const int64_t* offsets_host, int32_t n_links,
                          int64_t max_abs, int32_t* status, int32_t* face_count, void* workspace, size_t workspace_bytes,
                          creg_stream_t stream);
int creg_lattice_hull_emit_i32(const int32_t* pts, int64_t n, const int64_t* offsets, int32_t n_links,
                               const int64_t* tri_offsets, int64_t n_tri, const double* origin, double voxel_size,
                               int32_t* triangles, float* stl_records, void* workspace, size_t workspace_bytes,
                               creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The `--normal` branch (mlp_reg.py:190-203, cluster_icp.py:49-62; CLI flag mlp_reg.py:399): Open3D normal estimation +
 * orientation, then sklearn k_means over [xyz | 0.5 * normal].
 *
 * creg_knn_normals_f64: for every point of X (n,3) fp64 its (up to) max_nn <= 32 nearest points, itself included, ascending
 * by (squared distance, index); radius > 0 keeps only squared distances < radius^2 (open3d KDTreeFlann::SearchHybrid), radius
 * <= 0 none (SearchKNN).  idx_out (n, max_nn) int32 (-1 past the count), cnt_out (n) int32, normals (n,3) fp64 -- any may be
 * NULL.  normals = PointCloud::EstimateNormals of those neighbourhoods: unit eigenvector of the smallest eigenvalue of their
 * covariance (raw-moment form), (0,0,1) for fewer than three neighbours; signs are NOT oriented (the host does that:
 * autourdf_amd/normals.py, orient_normals_consistent_tangent_plane).  An exactly diagonal covariance gives the axis of its
 * smallest entry: z whenever z is among the smallest, y when only x and y tie.  A covariance that is exactly 0 gives (0,0,1).
 * n < 1 (an empty cloud), max_nn < 1 or max_nn > 32 return CREG_EINVAL with creg_last_error() set and launch nothing; the
 * Python wrapper (ops.knn_normals) raises RuntimeError with that text. */
int creg_knn_normals_f64(const double* X, int64_t n, double radius, int32_t max_nn, int32_t* idx_out, int32_t* cnt_out,
                         double* normals, creg_stream_t stream);
/* sklearn.cluster.k_means(X, init=<array>, n_clusters=k, n_init=1) over DIM-dimensional features (dim = 6: the --normal
 * branch's [xyz | 0.5 n]; 3 also accepted), k <= n < 2^24, k <= 128, one workgroup (labels in LDS up to 16384 points, in the
 * workspace above), no host sync.  X (n,dim), init (k,dim),
 * centers (k,dim) fp64; labels (n) int32; inertia (1) fp64; n_iter (1) int32; tol_rel = 1e-4 in the reference.
 * workspace: creg_kmeans_nd_workspace_bytes(n). */
size_t creg_kmeans_nd_workspace_bytes(int64_t n);
int creg_kmeans_lloyd_nd_f64(const double* X, int64_t n, int32_t dim, const double* init, int32_t k, int32_t max_iter,
                             double tol_rel, double* centers, int32_t* labels, double* inertia, int32_t* n_iter,
                             void* workspace, size_t workspace_bytes, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * N4  synthetic frames from a URDF + triangle meshes (the data side: Sim/sim_data.py:246-370 renders and
 * fuses depth images of the PyBullet model; here the mesh surfaces are sampled directly).
 * tri (n_tri,3,3) fp64 triangles in their link's frame, cum_area (n_tri) inclusive prefix sum of their
 * areas, tri_link (n_tri) link index, link_T (n_links,4,4) link poses of the current joint state,
 * u (n,3) uniforms in [0,1).  out (n,3) world points, link_out (n) optional link index per point. */
int creg_sample_mesh_f64(const double* tri, const double* cum_area, const int32_t* tri_link, int32_t n_tri,
                         const double* link_T, int32_t n_links, const double* u, int64_t n, double* out,
                         int32_t* link_out, creg_stream_t stream);

/* Camera-ring visibility of sampled surface points: what the reference's rendered depth cameras impose on its frames
 * (Sim/sim_data.py:88-116 camera ring, :246-306 depth images -> point clouds).  The posed triangles are rasterised into one
 * fp64 depth buffer per camera (width x height, pinhole, vertical fov `fov_deg`, linear depth along the view axis, minimum at
 * the pixel centres); visible[i] = 1 when point i projects into some camera's image between near and far and lies no more
 * than `eps` behind that camera's buffer at its pixel.  cams (n_cams,12) fp64 = eye | forward | right | up.
 * workspace: creg_visibility_workspace_bytes(n_cams, width, height) (the depth buffers). */
size_t creg_visibility_workspace_bytes(int32_t n_cams, int32_t width, int32_t height);
int creg_visibility_f64(const double* tri, const int32_t* tri_link, int32_t n_tri, const double* link_T, int32_t n_links,
                        const double* cams, int32_t n_cams, double fov_deg, double aspect, double near_val, double far_val,
                        int32_t width, int32_t height, const double* pts, int64_t n, double eps, uint8_t* visible,
                        void* workspace, size_t workspace_bytes, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Depth-camera frames (Sim/sim_data.py:283-329: one depth image per camera, every pixel back-projected, the per-camera
 * clouds fused; with a ground, Open3D's segment_plane removes it per camera, :311-319).
 *
 * creg_raster_depth_f64: the clear and raster passes of creg_visibility_f64 alone (the same kernels, no query points):
 * depth (n_cams,height,width) fp64, linear depth along the view axis at the pixel centres, +inf where nothing was drawn. */
int creg_raster_depth_f64(const double* tri, const int32_t* tri_link, int32_t n_tri, const double* link_T, int32_t n_links,
                          const double* cams, int32_t n_cams, double fov_deg, double aspect, double near_val, double far_val,
                          int32_t width, int32_t height, double* depth, creg_stream_t stream);
/* Every finite pixel (c, y, x) of depth (n_cams,height,width) becomes one world point, the inverse of the projection above at
 * the pixel centre:  nx = ((x + 0.5) / width - 0.5) * 2,  ny = ((1 - (y + 0.5) / height) - 0.5) * 2,
 *   xc = nx * ((d * tan(fov / 2)) * aspect),  yc = ny * (d * tan(fov / 2)),
 *   p = ((eye + d * forward) + xc * right) + yc * up      -- in exactly this order, no contraction.
 * The rows are ordered camera-major, then row-major pixels: a count, an exclusive scan and a scatter, no atomics; the
 * result is a pure function of the buffers.  Two calls, because the number of points is only known on the device:
 *   creg_depth_points_count_f64 -> offsets (n_cams + 1) int64 on the device: camera c owns rows offsets[c]:offsets[c+1];
 *                                  the per-block offsets stay in the workspace;
 *   creg_depth_points_f64       -> points (capacity,3) fp64 from the SAME depth and workspace; capacity is the caller's
 *                                  read of offsets[n_cams] (rows at or past capacity are dropped, never written).
 * 1 <= n_cams <= 65535, width * height < 2^31.  workspace: creg_depth_points_workspace_bytes(n_cams, width, height). */
size_t creg_depth_points_workspace_bytes(int32_t n_cams, int32_t width, int32_t height);
int creg_depth_points_count_f64(const double* depth, int32_t n_cams, int32_t width, int32_t height, int64_t* offsets,
                                void* workspace, size_t workspace_bytes, creg_stream_t stream);
int creg_depth_points_f64(const double* depth, const double* cams, int32_t n_cams, double fov_deg, double aspect,
                          int32_t width, int32_t height, const void* workspace, size_t workspace_bytes, double* points,
                          int64_t capacity, creg_stream_t stream);
/* Batched RANSAC plane segmentation (Open3D's PointCloud::segment_plane: distance_threshold, ransac_n, num_iterations) over
 * n_segments segments of one packed cloud: points (n,3) fp64, offsets (n_segments + 1) int64, segment s = rows
 * offsets[s]:offsets[s+1] (offsets outside [0, n] or running backwards are clamped).  samples (n_segments,n_hyp,ransac_n)
 * int64: the hypotheses' point indices RELATIVE to their segment's start, drawn by the caller (the library draws no random
 * numbers; an index may repeat within a hypothesis).  1 <= n < 2^31, n_hyp >= 1, 3 <= ransac_n <= 16, threshold > 0.
 *   fit     per hypothesis the least-squares plane through its samples: centroid (sum in sample order / ransac_n) and the
 *           unit eigenvector of the smallest eigenvalue of their scatter C (sums of centred products in sample order; the 3x3
 *           solver of creg_knn_normals_f64), signed so that its component of largest magnitude is positive (ties: lowest
 *           index); d = -((a cx + b cy) + c cz).
 *           Rank test: a fit is INVALID when  e2(C) <= 1e-12 * trace(C)^2,  e2 = (C00 C11 - C01^2) + (C00 C22 - C02^2) +
 *           (C11 C22 - C12^2) the sum of the principal 2x2 minors (= l0 l1 + l0 l2 + l1 l2 of the eigenvalues): the samples
 *           deviate from one line by less than about 1e-6 of their extent -- all identical (C = 0), two distinct points,
 *           exactly collinear ones (rounding leaves e2 / trace^2 near 1e-16).  Also invalid: an index outside the segment
 *           (nothing is read), non-finite moments, a segment of fewer than ransac_n points.  An invalid hypothesis has a
 *           plane of NaN and counts 0.
 *   count   a point is an inlier when fabs(((a*x + b*y) + c*z) + d) < threshold, in this operation order; exact integers.
 *   select  the valid hypothesis with the largest count, the smallest index among equals.
 *   refit   the least-squares plane through the best hypothesis's inliers (centroid, then the scatter about it; fixed
 *           reduction trees: two runs are identical), same sign rule.  If those inliers fail the rank test, or there are
 *           none, the best hypothesis's own plane is returned.
 * Outputs: plane (n_segments,4) the refit; mask (n) uint8 the inliers of the BEST HYPOTHESIS (not re-evaluated against the
 * refit; 0 outside every segment); count (n_segments) int64 their number; best (n_segments) int32; hyp_planes
 * (n_segments,n_hyp,4) fp64 and hyp_counts (n_segments,n_hyp) int32, either may be NULL.  A segment without a valid
 * hypothesis (an empty one included) has count 0, best -1, a plane of zeros and no mask bits.  No early termination: all
 * n_hyp hypotheses are always evaluated.  workspace: creg_segment_plane_workspace_bytes(n, n_segments, n_hyp). */
size_t creg_segment_plane_workspace_bytes(int64_t n, int32_t n_segments, int32_t n_hyp);
int creg_segment_plane_f64(const double* points, int64_t n, const int64_t* offsets, int32_t n_segments, const int64_t* samples,
                           int32_t n_hyp, int32_t ransac_n, double threshold, double* plane, uint8_t* mask, int64_t* count,
                           int32_t* best, double* hyp_planes, int32_t* hyp_counts, void* workspace, size_t workspace_bytes,
                           creg_stream_t stream);

/* Batched forward kinematics of a URDF joint table: every link pose of n_poses joint states in one launch (the evaluation
 * stage, Sim/evaluation.py:84-224 and :228-310, where PyBullet poses the robots one state at a time).
 * The table is in TOPOLOGICAL order -- a joint's parent link is `root` or the child of an earlier joint -- and holds, per
 * joint: parent / child (n_joints) link indices in [0, n_links), type (n_joints) 0 fixed, 1 revolute or continuous,
 * 2 prismatic, origin (n_joints,4,4) the joint frame in the parent link (translation already scaled), axis (n_joints,3)
 * UNIT axis in the joint frame.  q (n_poses,n_joints) joint values in the table's order, base (4,4) the root link's pose.
 * Poses are affine: bottom rows are taken as 0 0 0 1.
 *   link_T (n_poses,n_links,4,4):  T_child = T_parent * origin * motion(q), motion = I + sin q K + (1 - cos q) K K for
 *                                  type 1 (K = [axis]x), a translation by axis * q for type 2, I for type 0; the root is
 *                                  `base`, a link no joint reaches is the identity.
 *   joint_lines (n_poses,n_joints,6), may be NULL: (T_parent * origin)[:3,3] | (T_parent * origin)[:3,:3] axis -- the
 *                                  joint frame's origin and the unit joint axis in the world.
 * A joint whose parent or child index is outside [0, n_links) is skipped (its line is 0).  n_joints, n_links, n_poses >= 1. */
int creg_urdf_fk_f64(const int32_t* parent, const int32_t* child, const int32_t* type, const double* origin,
                     const double* axis, int32_t n_joints, int32_t n_links, int32_t root, const double* q,
                     int32_t n_poses, const double* base, double* link_T, double* joint_lines, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Self-collision of posed link meshes: all listed link pairs of all poses in one call, triangle mesh against triangle mesh.
 * The reference's generator asks PyBullet for self contacts and abandons the sequence at the first one
 * (Sim/sim_data.py:200-208, :276-281): convex hulls of the <collision> geometry with Bullet's margins, after a physics step.
 * PyBullet is not part of this build, so that check can NOT be pinned and is not imitated; the contract below is this
 * project's own.
 *   geometry   tri (n_tri,9) fp64: triangles in link frames (the <visual> triangles the frames are made of); link l owns rows
 *              tri_start[l] .. tri_start[l+1] (tri_start (n_links+1) int64, non-decreasing, 0 .. n_tri; values outside are
 *              clamped, nothing outside tri is read).  link_T (n_poses,n_links,16): row-major 4x4 poses, bottom row unread.
 *   vertex     w_i = ((R_i0*v_0 + R_i1*v_1) + R_i2*v_2) + t_i   -- in exactly this order, no contraction.
 *   pair       triangles (a, b) collide iff (1) their posed axis-aligned boxes overlap -- the box is the exact min / max of
 *              the three posed vertices, closed comparisons lo_a <= hi_b && lo_b <= hi_a on all three axes -- and (2) some
 *              edge of one properly pierces the other: the three edges of a against b and the three of b against a.
 *   piercing   orient(p,q,r,s) = ((u x v)_x*w_x + (u x v)_y*w_y) + (u x v)_z*w_z with u = q-p, v = r-p, w = s-p and
 *              (u x v) = (u_y*v_z - u_z*v_y, u_z*v_x - u_x*v_z, u_x*v_y - u_y*v_x).  Edge (p,q) properly pierces (a,b,c) when
 *              orient(a,b,c,p) and orient(a,b,c,q) have strictly opposite signs AND orient(p,q,a,b), orient(p,q,b,c),
 *              orient(p,q,c,a) are all > 0 or all < 0.  A zero anywhere is "no": touching, an edge through a vertex or
 *              through an edge, and coplanar overlap are not collisions; links mounted flush do not collide.  A mesh wholly
 *              INSIDE another is not detected here (no edge pierces a face): creg_mesh_contain_f64 below detects it when asked.
 *   culling    link boxes, boxes of 256-triangle chunks and tile union boxes are exact min / max of the same posed vertices,
 *              so with (1) in the contract they are exactly conservative: culling changes no output.
 * pairs (n_pairs,2) int32 link indices; which pairs to test (adjacent links intersect at every pose and are left out by the
 * caller: UrdfRobot.collision_pairs).  Outputs:
 *   count (n_poses,n_pairs) int32     colliding triangle pairs (a in link pairs[m][0], b in link pairs[m][1]); there is no early
 *                                     exit on the first hit.
 *   first (n_poses,n_pairs,2) int32   the lexicographically smallest such (a, b), rows of tri, or (-1,-1).
 *   link_box (n_poses,n_links,6)      min xyz | max xyz of the link's posed vertices, +inf | -inf for a link without triangles;
 *                                     may be NULL.
 * A pair that names a link outside [0, n_links), or one link twice, gives count 0 and (-1,-1).  n_pairs == 0 is valid and
 * fills link_box only.  Only integer atomics (add, 64-bit min of (a << 32) | b): two runs are identical.
 * CREG_EINVAL, nothing launched: n_poses < 1, n_pairs < 0, n_links < 1 or > 65535, n_tri < 0 or >= 2^31, a workspace smaller
 * than creg_mesh_collide_workspace_bytes(n_tri, n_links, n_poses, n_pairs) (posed vertices, chunk and link boxes, keys), which
 * is 0 for n_tri < 0 or >= 2^31, n_links < 1, n_poses < 1 and n_pairs < 0.
 * Limits: colliding triangle pairs per link pair and pose < 2^31. */
size_t creg_mesh_collide_workspace_bytes(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pairs);
int creg_mesh_collide_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T, int32_t n_links,
                          int64_t n_poses, const int32_t* pairs, int64_t n_pairs, int32_t* count, int32_t* first,
                          double* link_box, void* workspace, size_t workspace_bytes, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Link clearance: for every listed link pair of every pose, in one call, the minimum squared distance between the two posed
 * triangle meshes and the triangle pair that attains it.  The collision margin of the frame generator rests on it (the reference
 * rejects near-touching poses through Bullet's margins, which are not imitated; this contract is the project's own).
 *   inputs     tri, tri_start (with its clamping), n_tri, link_T, n_links, n_poses, pairs, n_pairs and link_box are exactly those
 *              of creg_mesh_collide_f64: the same posed vertices w_i, the same exact min / max boxes.  d_max >= 0 may be +inf.
 *   max, min   below, max(x, y) and min(x, y) are taken of operands that are never NaN for finite vertices; lo - hi of an empty
 *              box (+inf | -inf) is +inf.
 *   box gap    gap2(a, b) = (g_x*g_x + g_y*g_y) + g_z*g_z,  g_k = max(0, max(lo_a[k] - hi_b[k], lo_b[k] - hi_a[k])).
 *   contributes   triangle pair (a, b) contributes iff gap2(box_a, box_b) <= d_max*d_max (boxes of the three posed vertices).
 *              This test is part of the contract.  Floating-point subtraction, max, the square of a non-negative and a sum in
 *              a fixed order are all monotone, so in floating point the gap between two enclosing boxes never exceeds the gap
 *              between the boxes they enclose: culling by link box, 256-triangle chunk box and tile union box with the same
 *              formula changes no output.
 *   d2(a, b)   0.0 when the pair collides by the mesh-collide predicate above (boxes meet, closed comparisons, AND an edge
 *              properly pierces); otherwise the minimum of 15 terms: pt_tri2(a_i; b_0,b_1,b_2) and pt_tri2(b_i; a_0,a_1,a_2)
 *              for i = 0,1,2, and seg_seg2(a_i, a_i'; b_j, b_j') for i, j = 0,1,2 with i' = (i+1) mod 3.  Squared distances; no
 *              square root anywhere.  dot(u,v) = (u_x*v_x + u_y*v_y) + u_z*v_z; clamp01(x) = 0 if x < 0, else 1 if x > 1, else x.
 *   pt_tri2(p; a,b,c)   ab = b-a, ac = c-a, ap = p-a, bp = p-b, cp = p-c; d1 = dot(ab,ap), d2 = dot(ac,ap), d3 = dot(ab,bp),
 *              d4 = dot(ac,bp), d5 = dot(ab,cp), d6 = dot(ac,cp).  The first of these that holds decides:
 *                1  d1 <= 0 && d2 <= 0                          -> dot(ap,ap)                       (vertex a)
 *                2  d3 >= 0 && d4 <= d3                         -> dot(bp,bp)                       (vertex b)
 *                3  d6 >= 0 && d5 <= d6                         -> dot(cp,cp)                       (vertex c)
 *              then with vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4:
 *                4  vc <= 0 && d1 >= 0 && d3 <= 0               -> den = d1 - d3;  v = d1/den if den > 0 else 0;  w = 0        (edge ab)
 *                5  vb <= 0 && d2 >= 0 && d6 <= 0               -> den = d2 - d6;  v = 0;  w = d2/den if den > 0 else 0        (edge ac)
 *                6  va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0 -> den = (d4 - d3) + (d5 - d6);  w = (d4 - d3)/den if den > 0
 *                                                                  else 0;  v = 1 - w                                          (edge bc)
 *                7  otherwise                                   -> s = (va + vb) + vc;  v = vb/s, w = vc/s if s > 0 else v = w = 0  (face)
 *              and for 4..7  q_k = p_k - ((a_k + ab_k*v) + ac_k*w),  result dot(q,q).  (The Voronoi regions of the triangle,
 *              Ericson's closest point on a triangle, with the vertex tests first.)  Every guard answers with a point of the
 *              triangle, so a degenerate triangle gives no NaN; its true distance comes from the seg_seg2 terms.
 *   seg_seg2(p1,q1; p2,q2)   u = q1-p1, v = q2-p2, r = p1-p2; a = dot(u,u), e = dot(v,v), f = dot(v,r), c = dot(u,r),
 *              b = dot(u,v).  The first that holds:
 *                1  a <= 0 && e <= 0   -> s = 0, t = 0
 *                2  a <= 0             -> s = 0, t = clamp01(f/e)
 *                3  e <= 0             -> t = 0, s = clamp01((0 - c)/a)
 *                4  otherwise          -> den = a*e - b*b;  s = clamp01((b*f - c*e)/den) if den > 0 else 0;  t = (b*s + f)/e;
 *                                         if t < 0: t = 0, s = clamp01((0 - c)/a);  else if t > 1: t = 1, s = clamp01((b - c)/a)
 *              x_k = (p1_k + u_k*s) - (p2_k + v_k*t), result dot(x,x).
 *   outputs    dist2 (n_poses,n_pairs) fp64: the minimum of d2 over the contributing pairs with a in link pairs[m][0] and b in
 *              link pairs[m][1]; +inf when none contributes.
 *              witness (n_poses,n_pairs,2) int32: the lexicographically smallest (a, b), rows of tri, among the contributing
 *              pairs whose d2 has exactly the bits of the minimum; (-1,-1) when none contributes.
 *              link_box as in creg_mesh_collide_f64; may be NULL.
 * A pair that names a link outside [0, n_links), or one link twice, gives +inf and (-1,-1).  n_pairs == 0 fills link_box only.
 * A value above d_max*d_max can appear: the box gap was small and the triangles farther apart; callers read it as "beyond the
 * margin".  If the true distance of two links is at most d_max, the pair that attains it contributes, so the result is then the
 * mesh distance.  As in mesh-collide, a mesh wholly INSIDE another is not detected here: it has a positive clearance
 * (creg_mesh_contain_f64 below detects it when asked).
 * Determinism: nothing is pruned by a running best (computed d2 and computed gap2 are different formulas) and there are no
 * floating-point atomics -- each block of the pair pass writes one (d2, key = a << 32 | b) partial into its own workspace slot
 * (pose, pair, block), a finishing pass takes the lexicographic minimum of at most 128 slots.  Two runs give the same bits and
 * the same witness, and a link pair alone in a call gives the same as among others.
 * CREG_EINVAL, nothing launched: the argument errors of creg_mesh_collide_f64 (n_poses < 1, n_pairs < 0, n_links < 1 or > 65535,
 * n_tri < 0 or >= 2^31, a null pointer, null pairs / dist2 / witness with n_pairs > 0, a workspace smaller than
 * creg_mesh_clearance_workspace_bytes(...): posed vertices, chunk and link boxes, the partials), and a NaN or negative d_max. */
size_t creg_mesh_clearance_workspace_bytes(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pairs);
int creg_mesh_clearance_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T, int32_t n_links,
                            int64_t n_poses, const int32_t* pairs, int64_t n_pairs, double d_max, double* dist2, int32_t* witness,
                            double* link_box, void* workspace, size_t workspace_bytes, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Point-to-mesh distance: for every point of every pose, in one call, the minimum squared distance to the pose's posed triangle
 * mesh and the triangle that attains it.  The check of a written URDF against the raw clouds rests on it, and the triangle's link
 * is a part segmentation of the cloud.  The reference has no such step; this contract is the project's own.
 *   inputs     tri, tri_start (with its clamping), n_tri, link_T, n_links, n_poses and link_box are exactly those of
 *              creg_mesh_collide_f64: the same posed vertices w_i in the same operation order, the same exact min / max boxes.
 *              pts (n_pts,3) fp64: WORLD points.  Pose p owns rows pt_start[p] .. pt_start[p+1] (pt_start (n_poses+1) int64,
 *              non-decreasing, 0 .. n_pts; each pose's two values are clamped into 0 .. n_pts the way tri_start's are, nothing
 *              outside pts, dist2 and tri_idx is touched).  d_max >= 0 may be +inf.
 *   live       a point is live iff none of its three coordinates is NaN (x == x on each).  A point that is not live has no
 *              contributing triangle.  The box of a live point is lo = hi = the point.
 *   box gap    gap2 of the clearance contract above; for a triangle's box and a point p it reads
 *              gap2(p, box) = (g_x*g_x + g_y*g_y) + g_z*g_z,  g_k = max(0, max(lo[k] - p[k], p[k] - hi[k])).
 *   contributes   triangle f of pose p contributes to live point i of pose p iff gap2(p_i, box_f) <= d_max*d_max, box_f the exact
 *              min / max box of the three posed vertices.  This test is part of the contract.  By the monotonicity stated in the
 *              clearance contract, culling by link box, by 256-triangle chunk box and by the union box of a tile of live points,
 *              with the box-box gap2 and the same d_max*d_max, drops no contributing triangle: culling changes no output.
 *   d2(i, f)   pt_tri2(p_i; a, b, c) of the clearance contract above, (a, b, c) the posed vertices of row f: its seven cases in
 *              that order, dot(u,v) = (u_x*v_x + u_y*v_y) + u_z*v_z, no contraction, no square root.  A zero-area triangle goes
 *              through the den > 0 and s > 0 guards like any other; every guard answers with a point of the triangle.
 *   outputs    per point: best = +inf, idx = -1; then the contributing triangles of its pose in ascending row order, each
 *              replacing (best, idx) by (d2, row) when d2 < best.  So
 *              dist2 (n_pts) fp64: the minimum of d2 over the contributing triangles, +inf when there is none;
 *              tri_idx (n_pts) int32: the smallest row of tri whose d2 has exactly the bits of that minimum, or -1.
 *              (A d2 that is not below +inf -- a point with an infinite coordinate -- leaves +inf and -1.)
 *              link_box as in creg_mesh_collide_f64; may be NULL.
 *              A row of pts that no pose owns is not written.  n_pts == 0 fills link_box only.
 * A value above d_max*d_max can appear: the box gap was small and the triangle farther away; callers read it as "beyond d_max".
 * If a point's true distance to the mesh is at most d_max, the triangle that attains it contributes, so the result is then the
 * distance to the mesh.  Nothing is pruned by a running best (computed d2 and computed gap2 are different formulas, so that could
 * change a tie): d_max is the cull.
 * Determinism: no atomics.  A point's two outputs are a function of its coordinates and of its pose's posed mesh alone: they do
 * not depend on the other points or poses of the call, on the order of pts, or on scheduling.
 * CREG_EINVAL, nothing launched: n_poses < 1, n_links < 1 or > 65535, n_tri < 0 or >= 2^31, n_pts < 0 or >= 2^31,
 * (n_pts >> 6) + n_poses >= 2^31, a null tri (with n_tri > 0), tri_start, link_T, pt_start or workspace, a null pts, dist2 or
 * tri_idx with n_pts > 0, a NaN or negative d_max, a workspace smaller than creg_point_mesh_workspace_bytes(...) (posed vertices,
 * chunk and link boxes; 0 for the counts refused here).  Poses are posed in slices of 65535. */
size_t creg_point_mesh_workspace_bytes(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pts);
int creg_point_mesh_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T, int32_t n_links,
                        int64_t n_poses, const double* pts, const int64_t* pt_start, int64_t n_pts, double d_max, double* dist2,
                        int32_t* tri_idx, double* link_box, void* workspace, size_t workspace_bytes, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Mesh cover: the transposed reduction of point-to-mesh distance.  For every posed triangle of every pose, in one call, the minimum
 * squared distance to the pose's points, the point that attains it and the number of points within d_max.  It sees what the other
 * direction cannot: mesh surface that no point lies near (a link posed where no cloud is, a link that exists twice, a bloated
 * mesh).  The reference has no such step; this contract is the project's own.
 *   inputs     tri, tri_start (with its clamping), n_tri, link_T, n_links, n_poses, pts, pt_start (with its clamping), n_pts, d_max
 *              and link_box are exactly those of creg_point_mesh_f64: the same posed vertices w_i in the same operation order, the
 *              same exact min / max boxes.  pt_row (n_pts) int32 may be NULL.
 *   live, box gap, contributes, d2(i, f)   word for word those of creg_point_mesh_f64: a point is live iff none of its coordinates
 *              is NaN; triangle f of pose p contributes to live point i of pose p iff gap2(p_i, box_f) <= d_max*d_max;
 *              d2(i, f) = pt_tri2(p_i; a, b, c) with its seven cases, no contraction, no square root.  The matrix d2 is the same;
 *              creg_point_mesh_f64 takes its minimum over the triangles for every point, this entry over the points for every
 *              triangle.
 *   label      label(i) = pt_row ? pt_row[i] : (int32) i.  A caller that reorders the points of a pose passes each point's own row
 *              here.  Labels are read, not checked; those of the live points of one pose are expected distinct and >= 0.
 *   outputs    (n_poses, n_tri), row-major.  For row f of pose p that some link owns: best = +inf, idx = -1, near = 0; then for
 *              every live point i of pose p to which f contributes, in any order,
 *                replace (best, idx) by (d2, label(i))  iff  d2 < best || (d2 == best && idx >= 0 && label(i) < idx)
 *                near += (d2 < +inf && d2 <= d_max*d_max)
 *              So
 *              dist2 fp64: the minimum of d2 over the points to which f contributes, +inf when there is none;
 *              pt_idx int32: the smallest label among the points whose d2 has exactly the bits of that minimum, or -1;
 *              n_near int32 (may be NULL): the number of points to which f contributes whose d2 is at most d_max*d_max, the
 *              triangle's support (with d_max = +inf: the pose's points with a finite d2).
 *              (A d2 that is not below +inf -- a point with an infinite coordinate -- replaces nothing and is not counted.)
 *              The replacement is the lexicographic minimum over (d2, label), which no order of the walk changes.
 *              link_box as in creg_mesh_collide_f64; may be NULL.
 *              A row of tri that no link owns is not written.  n_pts == 0 writes +inf / -1 / 0 to every owned row and fills
 *              link_box.  tri_start is expected to run 0 .. n_tri without decreasing; with another one nothing outside the arrays
 *              is touched, and which rows count as owned is not defined.
 * A value above d_max*d_max can appear: the box gap was small and the point farther away; callers read it as "beyond d_max".  If a
 * triangle's true distance to the pose's points is at most d_max, the point that attains it contributes.  Nothing is pruned by a
 * running best: d_max is the cull.
 * Culling: by the monotonicity stated in the clearance contract, culling with the box-box gap2 and the same d_max*d_max by the
 * union box of a tile of 64 live points against the 256-triangle chunk box (a chunk box lies inside its link's box, so a test
 * against the link box skips nothing more) drops no contributing pair: culling changes no output.
 * Determinism: no atomics, floating-point or integer.  The outputs of a pose are a function of its set of (point, label) pairs and
 * of its posed mesh alone: they do not depend on the order of pts, on the other poses of the call, or on scheduling; two runs give
 * the same bits.
 * CREG_EINVAL, nothing launched: n_poses < 1, n_links < 1 or > 65535, n_tri < 0 or >= 2^31, n_pts < 0 or >= 2^31,
 * (n_pts >> 6) + n_poses >= 2^31, n_poses * n_tri > 2^56 (the (pose, row) offsets are 64-bit, and 72 bytes of posed vertices per
 * row must stay inside 64 bits too), a null tri (with n_tri > 0), tri_start, link_T, pt_start or workspace, a null pts with
 * n_pts > 0, a null dist2 or pt_idx with n_tri > 0, a NaN or negative d_max, a workspace smaller than
 * creg_mesh_cover_workspace_bytes(...): the posing stage's posed vertices, chunk and link boxes, then 48 bytes (one box) per
 * point-tile slot, (n_pts >> 6) + n_poses slots; 0 for the counts refused here.  Poses are worked in slices of 65535. */
size_t creg_mesh_cover_workspace_bytes(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pts);
int creg_mesh_cover_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T, int32_t n_links,
                        int64_t n_poses, const double* pts, const int64_t* pt_start, const int32_t* pt_row, int64_t n_pts,
                        double d_max, double* dist2, int32_t* pt_idx, int32_t* n_near, double* link_box, void* workspace,
                        size_t workspace_bytes, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Pose-fit system: from the correspondences of creg_point_mesh_f64 (every point's nearest triangle, hence its link), per pose the
 * Gauss-Newton system of fitting the robot's base pose and joint values to that pose's cloud.  The parameters of a pose are
 * D = 6 + n_joints numbers: a rotation vector about center_p (0..2), a translation (3..5) and one value per joint of the table
 * (6 + j).  The reference has no such step; this contract is the project's own.
 *   inputs     tri, tri_start (with its clamping), n_tri, link_T (n_poses,n_links,16), n_links, n_poses, pts, pt_start (with its
 *              clamping), n_pts and d_max are exactly those of creg_point_mesh_f64.
 *              tri_idx (n_pts) int32: the rows that entry returned; -1 or any value outside [0, n_tri) means no correspondence.
 *              parent, child, type, origin (n_joints,4,4), axis (n_joints,3), n_joints: the joint table of creg_urdf_fk_f64.
 *              chain (n_links) uint64: bit j is set iff joint j lies on the path from the root to link l (the caller builds it
 *              from the table; a joint with a parent or child index outside [0, n_links) sets no bit, as the forward kinematics
 *              skips it).  center (n_poses,3): the point the base rotation turns about.
 *   limit      D = 6 + n_joints <= 64.
 *   frames     per pose and joint, once:  W = link_T[p, parent[j]] * origin[j]  as an affine 3x4 product, the pose on the left:
 *              W_rc = (T_r0*O_0c + T_r1*O_1c) + T_r2*O_2c, and + T_r3 for c = 3;  o_j = W[:3,3];
 *              a_j[r] = (W_r0*axis_0 + W_r1*axis_1) + W_r2*axis_2.  A joint with a parent or child outside [0, n_links) has
 *              o_j = a_j = 0 (and no chain bit).
 *   contributes   point i of pose p contributes iff (1) it is live (x == x on each coordinate), (2) 0 <= f = tri_idx[i] < n_tri,
 *              (3) with l the largest link index whose clamped tri_start[l] is <= f (a bisection), f lies in link l's clamped
 *              rows, and (4) dot(r, r) <= d_max*d_max for the residual r below (false for a NaN; a point with an infinite
 *              coordinate has tri_idx -1 from creg_point_mesh_f64).
 *   residual   (a, b, c) = the three vertices of row f posed by link_T[p, l] with the vertex formula of creg_mesh_collide_f64,
 *              in the thread, so their bits are the posing stage's.  r = pt_tri_vec(p_i; a, b, c): the vector whose dot
 *              pt_tri2 returns -- ap, bp, cp for cases 1, 2, 3, and q for cases 4..7 -- chosen by the same seven cases in the
 *              same order with the same operations.  dot(r, r) has the bits of creg_point_mesh_f64's dist2 for that row.  The
 *              closest point is  c_k = p_i[k] - r_k.
 *   columns    3-vectors J_k of a contributing point of link l, with u x v = (u_y*v_z - u_z*v_y, u_z*v_x - u_x*v_z,
 *              u_x*v_y - u_y*v_x) and differences taken per component first:
 *                k = 0..2   e_k x (c - center_p), written out: (0, -v_z, v_y), (v_z, 0, -v_x), (-v_y, v_x, 0) for v = c - center_p
 *                k = 3..5   e_(k-3)
 *                k = 6 + j  a_j x (c - o_j) for type 1,  a_j for type 2,  when bit j of chain[l] is set
 *              and the zero vector otherwise (type 0 or any other type, or bit j not set).
 *   outputs    per pose, sums over its contributing points with dot(u,v) = (u_x*v_x + u_y*v_y) + u_z*v_z:
 *              H (n_poses,D,D) fp64: H[a][b] = sum dot(J_a, J_b), stored in full; H[a][b] and H[b][a] carry the same bits.
 *              g (n_poses,D) fp64: g[a] = sum dot(J_a, r).      cost (n_poses) fp64: sum dot(r, r).
 *              n (n_poses) int64: the number of contributing points.
 *              A pose with no contributing point (an empty one included) gets zeros.  The step that lowers the cost solves
 *              H delta = g: moving the model by delta moves c by J delta.
 *   order      a pose's rows are cut into tiles of 32 in row order from its first row.  Within a tile, every entry is summed from
 *              0.0 over the tile's rows in ascending order, a row that does not contribute (or lies past the pose's end) adding
 *              an exact zero.  The tiles' partials are then added in ascending tile order into four running sums, tile t into sum
 *              t mod 4, and the entry is (s0 + s1) + (s2 + s3).  n is summed the same way in fp64, exact below 2^53.
 * Determinism: no floating-point atomics; the order above depends on the pose's own row count alone.  Two runs give the same
 * bits, and a pose alone in a call gives the bits it has among others.
 * CREG_EINVAL, nothing launched: n_poses < 1, n_links < 1 or > 65535, n_tri < 0 or >= 2^31, n_pts < 0 or >= 2^31,
 * (n_pts >> 5) + n_poses >= 2^31, n_joints < 0 or 6 + n_joints > 64, a null tri (with n_tri > 0), tri_start, link_T, pt_start,
 * chain, center, H, g, cost, n or workspace, a null pts or tri_idx with n_pts > 0, a null table array with n_joints > 0, a NaN
 * or negative d_max, a workspace smaller than creg_pose_fit_workspace_bytes(n_poses, n_pts, n_joints) (the joint frames and one
 * partial of D*D + D + 2 doubles per tile slot; 0 for the counts refused here). */
size_t creg_pose_fit_workspace_bytes(int64_t n_poses, int64_t n_pts, int32_t n_joints);
int creg_pose_fit_system_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T, int32_t n_links,
                             int64_t n_poses, const double* pts, const int64_t* pt_start, int64_t n_pts, double d_max,
                             const int32_t* tri_idx, const int32_t* parent, const int32_t* child, const int32_t* type,
                             const double* origin, const double* axis, int32_t n_joints, const uint64_t* chain,
                             const double* center, double* H, double* g, double* cost, int64_t* n, void* workspace,
                             size_t workspace_bytes, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Link moments: from the same correspondences, per pose and link the 16 sums that every least-squares problem whose columns are
 * rigid twist fields is a small product around.  Restricted to the points of one link, a column of the pose-fit system above, or
 * of any refinement of the joint frames, moves the closest point c by Omega x (c - rho) + V; with d = c - rho the normal system
 * is  H[a][b] = Omega_a^T (tr(S2) I - S2) Omega_b + (Omega_a x S1).V_b + (Omega_b x S1).V_a + n V_a.V_b,
 * g[a] = Omega_a.Sx + V_a.Sr  summed over the links, for S2 = sum d d^T, S1 = sum d, Sx = sum d x r, Sr = sum r and the count n.
 * The sums do not depend on the parameter count.  The reference has no such step; this contract is the project's own.
 *   inputs     tri, tri_start (with its clamping), n_tri, link_T, n_links, n_poses, pts, pt_start (with its clamping), n_pts,
 *              d_max and tri_idx are exactly those of the pose-fit entry above.  There is no joint table and no limit on a
 *              parameter count.  ref (n_poses,n_links,3) fp64: the point rho the moments of (p, l) are taken about.
 *   contributes, residual   word for word those of the pose-fit entry: the same four conditions, the same bisection for the link
 *              l, the vertices posed in the thread, r = pt_tri_vec(p_i; a, b, c), the test dot(r, r) <= d_max*d_max, c_k =
 *              p_i[k] - r_k.  dot(r, r) has the bits of the point-mesh entry's dist2 for that row.
 *   terms      of a contributing row of (p, l), with d_k = c_k - ref[p,l][k] per component and dot and x as written above, single
 *              operations, no contraction, in this order:
 *                0..5    d_x*d_x, d_x*d_y, d_x*d_z, d_y*d_y, d_y*d_z, d_z*d_z
 *                6..8    d_x, d_y, d_z
 *                9..11   (d x r)_x, (d x r)_y, (d x r)_z
 *                12..14  r_x, r_y, r_z
 *                15      dot(r, r)
 *   outputs    mom (n_poses,n_links,16) fp64: the 16 sums in that order over the contributing rows of (p, l).
 *              cnt (n_poses,n_links) int64: their number.  Every (p, l) is written, with zeros where nothing contributes.
 *   order      a pose's rows are cut into tiles of 64 in row order from its first row.  Within a tile, every sum of (p, l) starts
 *              from 0.0 and runs over the tile's rows in ascending order; a row that does not contribute to (p, l) is skipped
 *              (adding +0.0 would give the same bits).  The tiles' partials are then added in ascending tile order into four
 *              running sums, tile t into sum t mod 4, and the result is (s0 + s1) + (s2 + s3).  cnt is summed the same way in
 *              fp64, exact below 2^53.
 * Determinism: no floating-point atomics.  Two runs give the same bits, a pose alone in a call gives the bits it has among
 * others, and the result of (p, l) does not depend on the rows of other links in the same tiles.
 * CREG_EINVAL, nothing launched: n_poses < 1, n_links < 1 or > 65535, n_tri < 0 or >= 2^31, n_pts < 0 or >= 2^31,
 * (n_pts >> 6) + n_poses >= 2^31, n_poses * n_links * 17 >= 2^39, a null tri (with n_tri > 0), tri_start, link_T, pt_start, ref,
 * mom, cnt or workspace, a null pts or tri_idx with n_pts > 0, a NaN or negative d_max, a workspace smaller than
 * creg_link_moments_workspace_bytes(n_poses, n_pts, n_links) (17 doubles per tile slot and link; 0 for the counts refused here). */
size_t creg_link_moments_workspace_bytes(int64_t n_poses, int64_t n_pts, int32_t n_links);
int creg_link_moments_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T, int32_t n_links,
                          int64_t n_poses, const double* pts, const int64_t* pt_start, int64_t n_pts, double d_max,
                          const int32_t* tri_idx, const double* ref, double* mom, int64_t* cnt, void* workspace,
                          size_t workspace_bytes, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Feature moments: the link moments above and, beside them, per pose and link the 21 sums of the curvature of the matched
 * feature.  Half the squared distance from a point to a flat feature -- a vertex, the line of an edge, the plane of a face -- has
 * an exact Hessian, the projector Pi onto the feature's normal space: I, I - t t^T (t the unit edge direction), n n^T (n the unit
 * normal).  Pi r = r, so the gradient sum J^T r and the cost are those of the link moments; only the curvature sum J^T Pi J differs
 * from the point-to-point sum J^T J, and restricted to the points of one link it is the 6 x 6 matrix M6 = sum A^T Pi A between the
 * twists (Omega, V): H[a][b] = sum_l (Omega_a | V_a)^T M6 (Omega_b | V_b).  The reference has no such step; this contract is the
 * project's own.
 *   inputs     exactly those of creg_link_moments_f64.
 *   contributes, residual   word for word those of the link-moments entry; which = the case pt_tri_vec returned for the row (1, 2, 3
 *              vertex a, b, c; 4, 5, 6 edge ab, ac, bc; 7 the face), (a, b, c) the posed vertices it was computed from.
 *   projector  of a contributing row, single operations with + - * / only (no square root), no contraction, dot and x as above:
 *                which 1..3   Pi = I (1.0 on the diagonal, 0.0 off it)
 *                which 4..6   e = b - a, c - a, c - b per component; ee = dot(e, e);
 *                             Pi_ij = delta_ij - (e_i*e_j)/ee  with delta_ij = 1.0 or 0.0, when ee > 0, else Pi = I
 *                which 7      N = (b - a) x (c - a); NN = dot(N, N);  Pi_ij = (N_i*N_j)/NN when NN > 0, else Pi = I
 *              (i <= j computed, Pi_ji = Pi_ij: the products commute bit for bit).  A zero-area triangle takes the guards.
 *   columns    d_k = c_k - ref[p,l][k] as in the link moments.  The six twist columns, as 3-vectors with their zeros:
 *                A_0 = (0, -d_z, d_y), A_1 = (d_z, 0, -d_x), A_2 = (-d_y, d_x, 0)   (e_k x d),   A_3, A_4, A_5 = e_0, e_1, e_2
 *              B_k[i] = dot(Pi_i, A_k) for Pi_i = (Pi_i0, Pi_i1, Pi_i2), every product and sum carried out, the zeros included.
 *   terms      0..15 the link-moments terms in that order; 16..36 the upper triangle of M6, row-major over a <= b
 *              ((0,0) (0,1) .. (0,5) (1,1) .. (5,5)): dot(A_a, B_b), again with the zeros; 37 the count's 1.0.
 *   outputs    mom (n_poses,n_links,16) fp64 and cnt (n_poses,n_links) int64: the contract, the order and the bits of
 *              creg_link_moments_f64.  fmom (n_poses,n_links,21) fp64: the 21 sums over the contributing rows of (p, l).  Every
 *              (p, l) is written, with zeros where nothing contributes.
 *   order      that of the link moments: tiles of 64 rows from the pose's first row; within a tile every sum of (p, l) starts
 *              from 0.0 and runs over the tile's rows in ascending order, the rows that do not contribute to (p, l) skipped; the
 *              tiles' partials in ascending tile order into four running sums, tile t into sum t mod 4, the result
 *              (s0 + s1) + (s2 + s3).
 * Determinism: no floating-point atomics.  Two runs give the same bits, a pose alone in a call gives the bits it has among
 * others, and the result of (p, l) does not depend on the rows of other links in the same tiles.
 * CREG_EINVAL, nothing launched: n_poses < 1, n_links < 1 or > 65535, n_tri < 0 or >= 2^31, n_pts < 0 or >= 2^31,
 * (n_pts >> 6) + n_poses >= 2^31, n_poses * n_links * 38 >= 2^39, a null tri (with n_tri > 0), tri_start, link_T, pt_start, ref,
 * mom, cnt, fmom or workspace, a null pts or tri_idx with n_pts > 0, a NaN or negative d_max, a workspace smaller than
 * creg_feature_moments_workspace_bytes(n_poses, n_pts, n_links) (38 doubles per tile slot and link; 0 for the counts refused
 * here). */
size_t creg_feature_moments_workspace_bytes(int64_t n_poses, int64_t n_pts, int32_t n_links);
int creg_feature_moments_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* link_T, int32_t n_links,
                             int64_t n_poses, const double* pts, const int64_t* pt_start, int64_t n_pts, double d_max,
                             const int32_t* tri_idx, const double* ref, double* mom, int64_t* cnt, double* fmom, void* workspace,
                             size_t workspace_bytes, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Containment:is a link wholly inside another?  For every listed link pair of every pose, in both directions and in one
 * call, the generalized winding number of one link's posed triangle mesh at a few points of the other.  It closes the hole the
 * two entries above share (no edge pierces a face when a mesh lies wholly inside another); the reference rejects such a pose
 * because Bullet's hulls overlap.  The winding number is +1 inside a closed outward-oriented mesh, -1 inside an inward-oriented
 * one, 0 outside a closed mesh, and degrades smoothly on a mesh with holes.  This contract is the project's own.
 *   inputs     tri, tri_start (with its clamping), n_tri, link_T, n_links, n_poses, pairs, n_pairs and link_box are exactly those
 *              of creg_mesh_collide_f64: the same posed vertices w_i in the same operation order, the same exact min / max link
 *              boxes.  pts (n_pts,3) fp64: query points in link frames; link l owns rows pt_start[l] .. pt_start[l+1]
 *              (pt_start (n_links+1) int64, clamped into 0 .. n_pts like tri_start).  A link owns 0 .. 16 points, and q_stride
 *              (1 .. 16) is at least every link's count.  A point is posed by the vertex formula with its own link's pose.
 *   direction  for pair m, direction 0 tests the points of link pairs[m][0] against the mesh of link pairs[m][1]; direction 1
 *              the points of pairs[m][1] against the mesh of pairs[m][0].
 *   gate       a posed point x is evaluated against link b iff lo_b[k] <= x[k] <= hi_b[k] on all three axes (closed
 *              comparisons, the exact link box).  Otherwise its winding is exactly 0.0 and nothing is summed.  The gate is part of
 *              the contract and the only cull: a chunk box cannot cull a winding sum.
 *   term       per posed triangle (v0,v1,v2) of link b:  a = v0 - x, b = v1 - x, c = v2 - x;  la = sqrt(dot(a,a)), lb and lc
 *              likewise;  det = dot(a, cross(b,c));  den = (((la*lb)*lc + dot(a,b)*lc) + dot(b,c)*la) + dot(c,a)*lb;
 *              omega = 2*atan2(det, den)  -- dot and cross as defined above, in exactly this order, no contraction; atan2 and
 *              sqrt are the device library's.  Finite inputs give no NaN; a triangle with two equal vertices gives exactly 0, a
 *              collinear one a value at rounding level.  A point ON the surface gives a finite value, but which one is outside
 *              what this contract promises.
 *   sum        per point, S = the terms of link b's triangles added in the fixed tree of creg_mesh_inertia_f64 (leaves in
 *              order, padded with zeros to a multiple of 256; per 256 leaves four 64-lane butterflies, then ((w0+w1)+w2)+w3; the
 *              chunk results are the leaves of the next level; at least one such level runs).  The tree depends on link b's
 *              triangle count alone.  w = S / (4*pi), and the point is inside iff fabs(w) > 0.5.
 *   outputs    inside (n_poses,n_pairs,2) int32: the number of inside points per direction.
 *              first (n_poses,n_pairs,2) int32: the smallest inside row of pts, or -1.
 *              winding (n_poses,n_pairs,2,q_stride) fp64, may be NULL: w of the link's points in their order; a slot beyond the
 *              link's count and a gated-out point hold 0.0.
 *              link_box as in creg_mesh_collide_f64; may be NULL.
 * A pair that names a link outside [0, n_links), or one link twice, gives 0, -1 and zeros.  n_pairs == 0 fills link_box only.
 * Every output element is written by every successful call.
 * Determinism: no floating-point atomics -- each block of the pair pass stores one partial per (pose, pair, direction, point,
 * chunk) into its own workspace slot, a finishing pass runs the upper tree levels.  Two runs give the same bits, and a pair alone
 * in a call gives the same bits as among others.
 * pt_start is read back by the host before anything is launched (the one stream synchronisation of this entry).
 * CREG_EINVAL, nothing launched: the argument errors of creg_mesh_collide_f64 (n_poses < 1, n_pairs < 0, n_links < 1 or > 65535,
 * n_tri < 0 or >= 2^31, a null pointer, null pairs / inside / first with n_pairs > 0), n_pts < 0 or >= 2^31, a null pts (with
 * n_pts > 0) or pt_start, q_stride outside 1 .. 16, a link that owns more points than q_stride (so more than 16), a workspace
 * smaller than creg_mesh_contain_workspace_bytes(...): posed vertices, chunk and link boxes and
 * n_poses * n_pairs * 2 * q_stride * max(1, ceil(n_tri/256)) partials.
 * Not detected: a shell of a link beyond the 16 points the caller chose (UrdfRobot.containment_points takes one point per
 * connected component, the largest first), and a point on the surface. */
size_t creg_mesh_contain_workspace_bytes(int64_t n_tri, int32_t n_links, int64_t n_poses, int64_t n_pairs, int32_t q_stride);
int creg_mesh_contain_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, const double* pts, const int64_t* pt_start,
                          int64_t n_pts, const double* link_T, int32_t n_links, int64_t n_poses, const int32_t* pairs,
                          int64_t n_pairs, int32_t q_stride, int32_t* inside, int32_t* first, double* winding, double* link_box,
                          void* workspace, size_t workspace_bytes, creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Mass properties of closed, outward-oriented link meshes: every link of a call in one set of launches, no host
 * synchronisation.  The reference writes mass 1.0, ixx = iyy = izz = 0.1 and the visual's origin into every <inertial> block
 * ("example values, adjust as needed", PointCloud/compute_joints.py:334-339); this contract is the project's own.
 *   geometry   tri (n_tri,9) fp64 and tri_start (n_links+1) int64 as creg_mesh_collide_f64 takes them (values outside
 *              0 .. n_tri are clamped, nothing outside tri is read); density (n_links) fp64.
 *   triangle   with r = the first vertex of the link's first triangle: a = v0 - r, b = v1 - r, c = v2 - r, e1 = b - a,
 *              e2 = c - a, s = (a + b) + c, cross(u,v) = (u_y*v_z - u_z*v_y, u_z*v_x - u_x*v_z, u_x*v_y - u_y*v_x),
 *              n = cross(e1,e2), g = cross(b,c), d = (a_x*g_x + a_y*g_y) + a_z*g_z, and the 14 terms
 *                0..2   n_x, n_y, n_z              3   sqrt((n_x*n_x + n_y*n_y) + n_z*n_z)              4   d
 *                5..7   d*s_x, d*s_y, d*s_z        8..13   d*(((s_i*s_j + a_i*a_j) + b_i*b_j) + c_i*c_j), ij = xx xy xz yy yz zz
 *              -- in exactly this order, no contraction.  The longest path of a term has 8 roundings (a_i, a_i + b_i, s_i,
 *              s_i*s_j, the three additions behind it, the product with d; d itself is 6 deep).
 *   sums       sums (n_links,14): the terms of the link's triangles added in a tree that depends on the link's triangle
 *              count alone.  Leaves are the triangles in order, padded with zeros to a multiple of 256; every 256 leaves go
 *              through: four groups of 64, each summed as a butterfly (x_i + x_(i^32), then ^16 ... ^1), then
 *              ((w0 + w1) + w2) + w3 -- depth 9.  The per-chunk results are the leaves of the next level, same tree, until
 *              one value is left; at least one such level runs.  Depth 9*(1 + max(1, ceil(log256(ceil(F_l/256))))), so with
 *              k = 8 + that depth:  |sum - exact| <= k * 2^-53 * sum|term|,  k = 26 for F_l <= 65536, 35 for F_l <= 2^24 and
 *              44 below 2^31: within 32 + ceil(log2 F_l) for every F_l >= 1.  This k counts the roundings of the longest
 *              single path; it is a working bound, not a proof.  A product's relative error is the sum of its factors', so
 *              to first order a term 8..13 carries d's 6 plus the bracket's 7 plus 1 = 14 roundings, not 8 (k = 32, 41, 50:
 *              still inside the cap), and both counts are relative to the factors' own absolute sums, which
 *              cancellation inside d can leave above |term|.  No floating-point atomics: two runs give the
 *              same bits, and a link gives the same bits alone in a call or among others.
 *              A link without triangles, or whose sum of d is 0, gets 14 zeros.
 *   derived    from the (possibly zeroed) sums S, in this order:
 *              volume = S4/6; area = S3/2; closure = sqrt((S0*S0 + S1*S1) + S2*S2)/S3 if S3 > 0 else 0; mass = density*volume;
 *              m_i = (S(5+i)/24)/volume; com (n_links,3) = r_i + m_i; C_ij = S(8+ij)/120 - (volume*m_i)*m_j;
 *              inertia (n_links,6) = ixx, ixy, ixz, iyy, iyz, izz of density*(tr(C) 1 - C) about com in the mesh's axes:
 *              density*(C_yy + C_zz), -(density*C_xy), -(density*C_xz), density*(C_xx + C_zz), -(density*C_yz),
 *              density*(C_xx + C_yy);
 *              principal (n_links,3) ascending eigenvalues of the inertia tensor and axes (n_links,3,3), row k the unit
 *              eigenvector of principal[k] (largest component positive for rows 0 and 1, row 2 = row 0 x row 1): eight
 *              sweeps of cyclic Jacobi rotations.
 *              For a link with zero sums volume, area, closure and mass are 0 and com, inertia, principal and axes are NaN.
 *              A negative volume (an inward-oriented mesh) is reported as it is.
 * CREG_EINVAL, nothing launched: n_links < 1 or > 65535, n_tri < 0 or >= 2^31, a null pointer, a workspace smaller than
 * creg_mesh_inertia_workspace_bytes(n_tri, n_links) (14 doubles per 256-triangle chunk: floor(n_tri/256) + n_links + 1 slots). */
size_t creg_mesh_inertia_workspace_bytes(int64_t n_tri, int32_t n_links);
int creg_mesh_inertia_f64(const double* tri, const int64_t* tri_start, int64_t n_tri, int32_t n_links, const double* density,
                          double* sums, double* volume, double* area, double* closure, double* mass, double* com,
                          double* inertia, double* principal, double* axes, void* workspace, size_t workspace_bytes,
                          creg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A1  the whole `train` loop (mlp_reg.py:17-152) as one device-resident plan: per epoch
 * pose -> sin/cos features -> MLP -> pose -> calculate_pc -> L1 Chamfer -> backward -> Adam ->
 * ReduceLROnPlateau, best-loss tracking and early stop, with no host round trip per epoch
 * (the reference syncs on loss.item() every epoch, mlp_reg.py:102).
 *
 * The reference's four --r choices (mlp_reg.py:64-90, models built at :276-291):
 * rot = 0: ROT == 'q'   with QRegMLP(True, hidden)  (model_utils.py:101-159)   pose row [t | quaternion], 7 -> 56 features
 * rot = 1: ROT == 'dq'  with DQRegMLP(hidden)       (model_utils.py:65-99)     dual quaternion, 8 -> 64 features, one decoder, ReLU
 * rot = 2: ROT == '6d'  with RRegMLP(hidden)        (model_utils.py:170-214)   [t | first two rows of R], 9 -> 72 features
 * rot = 3: ROT == 'rpy' with RegMLP(True, hidden)   (model_utils.py:216-281)   [t | XYZ Euler angles], 6 -> 48 features, Tanh after
 *                                                                              decoder_2 (the reference builds RegMLP(6, 3):
 *                                                                              hidden 3 -- run zero-padded at 64, see `hidden`)
 * Parameter order in `params` (torch nn.Linear layout, weight (out,in) row-major):
 *   rot 0, 2, 3: encoder.0.{weight,bias}, decoder_1.0.{w,b}, decoder_1.2.{w,b}, decoder_2.0.{w,b},
 *          decoder_2.2.{w,b}                                        (10 tensors)
 *   rot 1: encoder.0.{w,b}, decoder.0.{w,b}, decoder.2.{w,b}        (6 tensors)
 */
typedef struct creg_train_shape {
    int32_t rot;          /* 0 'q', 1 'dq', 2 '6d', 3 'rpy' */
    int32_t k;            /* clusters (poses), <= 256 (k_bd's LDS tiles: '6d' <= 227, <= 193 at hidden 512) */
    int32_t hidden;       /* hidden_dim in {64, 128, 256, 512} (512 in the reference); any other width <= 512: pass the next of these
                             and the parameters zero-padded to it -- exactly equivalent, see autourdf_amd/ops.py::TrainPlan */
    int32_t epochs;       /* 300 in the reference (mlp_reg.py:60) */
    int64_t n_pred;       /* sum of cluster sizes */
    int64_t n_tgt;        /* points in the target frame */
    int32_t use_graph;    /* 0: eager launches; 1: hipGraph of 50 epochs per launch; n > 1: n epochs per graph */
    int32_t batch;        /* independent problems (sequences) advanced per launch; 0 or 1 = one */
    int32_t graph_branches; /* how the problems of a batch share the GPU: the batch is cut into contiguous groups ("chains") whose
                               epochs run concurrently in different hardware queues, so that one group's latency-bound kernels
                               overlap another's.  0 = auto: chain streams (below), 1 chain up to 4 problems, 2 for 5-7, 3 from 8;
                               3 from 3 problems on when n_tgt > 4096.  -n: n CHAIN STREAMS -- every chain a linear graph on its own
                               stream (chain 0 on the caller's), forked / joined once per train by events; under 1.5 ms of host
                               time per train.  +n: n parallel branches inside ONE graph (rounds 2-3; the runtime enqueues every
                               node of such a graph from the host at each replay: 9-14 ms per train).  At most 3 chains are
                               useful (a fourth needs a fifth hardware queue).  Results do not depend on it. */
    int32_t nn_search;    /* 0 = auto: the nearest-neighbour searches run over k-d leaf blocks with boxes (exact
                             pruning) when n_tgt <= 65536 (four chunks of 16384 sorted per workgroup) and, for the
                             target -> predicted direction, when the predicted cloud fits 512 blocks (n_pred / 64 + k,
                             or n_pred / 256 + k above 4096 targets) with n_pred < 65535; 1 = exhaustive in both
                             directions; 2 = as 0, but always the four-queries-per-wave search of rounds 2-4.  Round 5: under 0,
                             frames of 4097..16384 target points (and a predicted cloud of at most 512 64-point blocks) take the
                             sixteen-queries-per-wave search (nn_l1.h: nn_l1_rows; franka shape 80.7 -> 104.2 frames/s).  Matches,
                             distances and the gradients of an epoch do not depend on it; the LOSS is summed per 16-slot group there
                             instead of per 32 original indices and can differ in its last bit -- and the loss feeds comparisons
                             (min_loss / best pose, ReduceLROnPlateau, early stop): a last-bit flip AT one of them changes lr or the
                             returned pose from there on, so trained parameters agree between searches only as far as no such
                             comparison is that close (none seen in the stress runs, not guaranteed).
                             creg_train_plan_info says what a plan chose (pruned_target_search is TRI-state: 0, 1, 2). */
} creg_train_shape;

typedef struct creg_train_args {
    const float* m;             /* (k,4,4) current poses */
    const float* y;             /* (n_tgt,3) target frame */
    const float* local_pts;     /* (n_pred,3) clusters in local frames, back to back */
    const int32_t* seg_offsets; /* (k+1) int32, DEVICE */
    float* const* params;       /* HOST array of 10 (rot 0, 2, 3) / 6 (rot 1) device pointers; updated in place */
    float lr;                   /* 2e-4 (Step) / 1e-4 (Anchor), mlp_reg.py:17,354 */
    float sched_factor;         /* 0.7 */
    int32_t sched_patience;     /* 5 */
    int32_t stop;               /* 200 */
    float* best_m;              /* (k,4,4) out */
    float* best_pred;           /* (n_pred,3) out: clusters at the best epoch, back to back */
    float* loss_hist;           /* (epochs) out, entries after an early stop are NaN; may be NULL */
    float* lr_hist;             /* (epochs) out (lr used by that epoch's Adam step); may be NULL */
    float* result;              /* (4) out: [min_loss, epochs_run, final_lr, best_epoch] */
    int32_t y_unchanged;        /* != 0: the caller guarantees that `y` holds the values it held in this plan's PREVIOUS run of this problem
                                   slot -- match() registers every frame twice, "Step" then "Anchor" (mlp_reg.py:338-356).  When every
                                   problem of a call says so the plan keeps the target frame's k-d leaf blocks (one bitonic sort per
                                   frame instead of one per train: 145 us at 4096 points, 673 us at 16384).  0 is always correct; since
                                   round 5 a non-zero value is VERIFIED on the device (a 64-bit position-dependent fingerprint of the staged
                                   frame against the one stored with the leaves): a frame that differs is sorted again, never searched
                                   through stale leaves. */
    int32_t reserved_;
} creg_train_args;

typedef struct creg_train_plan creg_train_plan;

/* What a plan decided from its shape (nothing here changes a result): which nearest-neighbour search each direction runs,
 * how many graph branches and problems per launch it uses.  A caller that sized its clouds beyond the pruned search's
 * limits sees it here instead of only in the timing. */
typedef struct creg_train_plan_info_t {
    int32_t pruned_target_search;     /* 1: predicted -> target search over k-d leaf blocks, four queries per wave; 2: sixteen queries per wave
                                         (both directions); 0: exhaustive (n_tgt > 65536 or nn_search = 1) */
    int32_t pruned_predicted_search;  /* 1: target -> predicted search over blocks; 0: exhaustive (more than 128 predicted blocks, ...) */
    int32_t graph_branches;           /* parallel chains in the captured graph */
    int32_t batch;                    /* problems the plan advances per run_batch call */
    int32_t epochs_per_graph;         /* 0: eager launches */
    int32_t nn_points_per_lane;       /* points per lane and block visit of the pruned search (1: 64-point blocks, 4: 256-point blocks) */
    int32_t nn_boxes_target;          /* boxes per lane of the search over the target frame (the k_nn_plan instance) */
    int32_t nn_boxes_predicted;       /* ... and over the predicted cloud */
    int32_t chain_probe_us;           /* chain streams (graph_branches <= 0, more than one chain), after the first run: the slowest joint run of two 150 us spin
                                         kernels on the caller's stream + the accepted chain streams, in us (< 250: they ran CONCURRENTLY, i.e. sit in different
                                         hardware queues); -1: no such stream was found and a chain shares a queue (its epochs then run after the other chain's);
                                         0: not probed (one chain, no run yet, or CREG_NO_QUEUE_PROBE=1) */
} creg_train_plan_info_t;

size_t creg_train_workspace_bytes(const creg_train_shape* shape);   /* covers shape.batch problems */
/* `workspace` (device, 256-byte aligned) must stay valid until creg_train_plan_destroy. */
int creg_train_plan_create(const creg_train_shape* shape, void* workspace, size_t workspace_bytes,
                           creg_train_plan** plan);
/* Enqueues the whole loop on `stream`; asynchronous (outputs are ready when the stream is). */
int creg_train_plan_run(creg_train_plan* plan, const creg_train_args* args, creg_stream_t stream);
/* Same for `n` == shape.batch independent problems of identical shape (K, N, hidden, epochs) advanced
 * together: every launch carries all of them in grid.z, so the latency-bound kernels of one sequence
 * overlap those of the others (sequences of a run are independent; frames of ONE sequence are not).
 * args[b] describes problem b; results are bit-identical to n separate creg_train_plan_run calls. */
int creg_train_plan_run_batch(creg_train_plan* plan, const creg_train_args* args, int32_t n, creg_stream_t stream);
int creg_train_plan_info(const creg_train_plan* plan, creg_train_plan_info_t* info);
int creg_train_plan_destroy(creg_train_plan* plan);

/* Round 6: a train continued from a caller-supplied state -- checkpoint / resume of `train`, and the hook the teacher-forced
 * late-epoch parity tests use (the reference's state entering epoch e, then ONE epoch of the plan).  What the reference keeps in Python
 * objects between epochs (mlp_reg.py:41-50 optimizer + scheduler, :96-119 the loop): torch.optim.Adam's exp_avg / exp_avg_sq per tensor
 * and its step count, ReduceLROnPlateau's best / num_bad_epochs / the current lr, train()'s own min_loss / count. */
typedef struct creg_train_state {
    float* const* exp_avg;      /* HOST array of device pointers: Adam's first moments, order and shapes of creg_train_args.params */
    float* const* exp_avg_sq;   /* ... second moments */
    double lr;                  /* the lr the NEXT optimizer step uses (optimizer.param_groups[0]['lr']) */
    double sched_best;          /* ReduceLROnPlateau.best (+inf before the first scheduler.step) */
    int32_t step;               /* optimizer steps taken so far */
    int32_t epochs_run;         /* epochs completed so far (= step unless stopped): the index the next loss is recorded at */
    int32_t sched_bad;          /* ReduceLROnPlateau.num_bad_epochs */
    int32_t count;              /* epochs since the loss last improved (mlp_reg.py:104-111) */
    int32_t best_epoch;         /* epoch min_loss was seen at; -1: none yet (then best_m / best_pred of the args are outputs only) */
    int32_t stopped;            /* != 0: the train had stopped early (the resumed epochs then change nothing) */
    float min_loss;             /* 1000 before the first epoch (mlp_reg.py:53) */
    int32_t reserved_;
} creg_train_state;
/* Runs `n_epochs` further epochs of problem `args` (slot 0 of the plan, eager launches) from `from`; from->step + n_epochs and
 * from->epochs_run + n_epochs must not exceed shape.epochs.  args->params: in (the parameters entering the resumed epochs) / out;
 * args->best_m / best_pred: in (when from->best_epoch >= 0) / out; loss_hist / lr_hist: entries [from->epochs_run, + n_epochs) are
 * written, the others are NaN.  exp_avg_out / exp_avg_sq_out (HOST arrays of device pointers, may be NULL): the moments after the
 * run; state_out (DEVICE, 12 doubles, may be NULL): [step, epochs_run, lr, sched_best, sched_bad, count, min_loss, best_epoch,
 * stopped, last_loss, 0, 0].  Asynchronous like creg_train_plan_run.  The next run_batch re-sorts its target frames. */
int creg_train_plan_resume(creg_train_plan* plan, const creg_train_args* args, const creg_train_state* from, int32_t n_epochs,
                           float* const* exp_avg_out, float* const* exp_avg_sq_out, double* state_out, creg_stream_t stream);

/* Test / profiling hook: run exactly one epoch's forward and return intermediates.
 * m2 (k,4,4), pred (n_pred,3), loss (1), grad_m2 (k,4,4: [dL/dR | dL/dt]); any may be NULL. */
int creg_train_plan_probe(creg_train_plan* plan, const creg_train_args* args, float* m2,
                          float* pred, float* loss, float* grad_m2, creg_stream_t stream);

/* Measurement hook: run n_epochs eagerly with a HIP event before / after each of the five kernels
 * of an epoch (order: head, nn_l1, gradc, bd, l2) on `stream`, synchronise, and write the
 * average microseconds per kernel to us_out (HOST, 16 floats): [0] 0, [1..5] event-bracketed per kernel in that order
 * (they include the dispatch latency of the launch, i.e. they are an upper bound of the kernel time),
 * [6] the nearest-neighbour kernel alone as 200 back-to-back launches between two events (kernel + launch gap),
 * [7] the problems that launch carries, [8] the backward launch k_bd the same way, [9] k_l2, [10] head, [11] gradc,
 * [12..15] reserved. */
int creg_train_plan_profile(creg_train_plan* plan, const creg_train_args* args, int32_t n_epochs,
                            float* us_out, creg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CREG_H */
