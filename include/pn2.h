/*
 * pn2.h -- C ABI of libpn2.so, the MI355X (gfx950) PointNet++ set-abstraction path.
 *
 * Every entry point:
 *   - takes plain pointers to caller-allocated DEVICE buffers (the caller's allocator owns all
 *     memory; nothing here allocates), element strides as int64, and a hipStream_t passed as
 *     void*;
 *   - is asynchronous on that stream and never synchronises the device, so it may be captured
 *     into a hipGraph;
 *   - returns PN2_OK (0) or a negative PN2_E* code; the message of the last failure on the
 *     calling thread is returned by pn2_last_error() (thread-local).
 *   - is re-entrant across host threads, as the reference's concurrent-inference demo
 *     /root/reference/mutilthreading/predict_test.py:44-63 requires: besides the caller's
 *     buffers the library holds only thread-local state (the error message, a thread's tuning
 *     copy, a thread's device error slots), the process-wide tuning keys (one atomic word per
 *     key) and the process-wide default error slot (kernels only OR into it; its reads are
 *     serialised).
 *
 * Reference interfaces replaced (file:line in /root/reference):
 *   pn2_fps_f32            farthest_point_sample            model/pointnet2_utils.py:47-68
 *   pn2_fps_ws_f32         the same, any N (workspace)       model/pointnet2_utils.py:47-68
 *   pn2_fps_host_ws_f32    the same, start drawn on the host model/pointnet2_utils.py:59
 *   pn2_ball_query_multi_i32  query_ball_point per MSG radius   model/pointnet2_utils.py:197-203
 *                          (+ index_points(points, fps_idx)  model/pointnet2_utils.py:106)
 *   pn2_ball_query_f32     query_ball_point + square_distance model/pointnet2_utils.py:70-90, 5-26
 *   pn2_pack_points_f32    torch.sum(points**2,-1) of square_distance model/pointnet2_utils.py:24-25
 *   pn2_square_distance_f32 square_distance                  model/pointnet2_utils.py:5-26
 *   pn2_index_points_f32   index_points                      model/pointnet2_utils.py:28-45
 *   pn2_group_f32          grouping of sample_and_group /    model/pointnet2_utils.py:107-116,
 *                          PointNetSetAbstractionMsg         model/pointnet2_utils.py:204-209
 *   pn2_group_backward_f32 the feature gradient of that grouping (autograd's backward of
 *                          index_points' advanced indexing)  model/pointnet2_utils.py:44
 *   pn2_pack_layer_f32    Conv2d(1x1)+BatchNorm2d(eval) params of the shared MLP
 *                                                            model/pointnet2_utils.py:150-156, 184-193
 *   pn2_sa_mlp_max_f32     grouped shared MLP (conv+bn+relu)* + max over the neighbourhood
 *                                                            model/pointnet2_utils.py:167-172, 211-218
 *   pn2_gemm_nt_f32 / pn2_gemm_nn_f32 / pn2_gemm_tn_f32
 *                          the shared MLP's 1x1 convs under autograd: forward, input gradient,
 *                          weight gradient, each sum in a fixed order
 *                                                            model/pointnet2_utils.py:167-172, 211-218
 *   pn2_fc_bn_forward_f32 / pn2_fc_bn_backward_f32
 *                          the heads' Linear + BatchNorm1d + ReLU under autograd, forward and
 *                          backward, each sum in a fixed order   model/pointnet2_cls_ssg.py:31-36;
 *                                                            translation_ssg.py:23-26
 *   pn2_fc_bn_forward_rows_f32 / pn2_fc_bn_backward_rows_f32
 *                          the same for batches above 64 rows (the scripts' --batch_size)
 *   pn2_transform_points_f32 / pn2_transform_points_backward_f32
 *                          torch.bmm of a T-Net's transform with the points under autograd
 *                                                            model/pointnet_utils.py:102-113, 120-123;
 *                                                            pose.py:50-69
 *   pn2_orthogonality_forward_f32 / pn2_orthogonality_backward_f32
 *                          feature_transform_reguliarzer     model/pointnet_utils.py:140-147
 *   pn2_bn_train_stats_f32 / pn2_bn_relu_apply_f32 (/ pn2_bn_train_forward_f32: both) /
 *   pn2_group_max_f32 / pn2_bn_relu_backward_f32
 *                          train-mode BatchNorm2d + ReLU + torch.max over K, forward and backward
 *                                                            model/pointnet2_utils.py:167-172, 211-221
 *                                                            (under autograd: train_rotation.py:99-133)
 *                          and the v1 shared MLPs' Conv1d + BatchNorm1d (+ ReLU) + max over N
 *                                                            model/pointnet_utils.py:31-35, 118-128
 *   pn2_bn_relu_group_max_f32 / pn2_bn_relu_backward_f32 with PN2_LAYER_FROZEN_STATS
 *                          eval-mode BatchNorm2d + ReLU + torch.max over K under autograd
 *                                                            model/pointnet2_utils.py:163-172, 211-221
 *                                                            (mutilthreading/predict_test.py:25-63)
 *   pn2_linear_rows_f32   eval Linear + BatchNorm1d (folded on the host) + ReLU of the FC tails
 *                                                            model/pointnet_utils.py:33-40;
 *                                                            pointnet_cls.py:26-28; rotation.py:45-49;
 *                                                            pointnet2_cls_ssg.py:32-34
 *   pn2_prepare_points_f64 the scripts' input preparation: provider.normalization + torch.Tensor
 *                          + provider.splice_torch + transpose (+ the translation heads' mean)
 *                                                            provider.py:5-21, 166-180;
 *                                                            test_translation.py:72-79
 *   pn2_prepare_train_points_f64  the same after the training scripts' augmentations
 *                          (random_point_dropout, random_scale_point_cloud, shift_point_cloud)
 *                                                            provider.py:131-164;
 *                                                            train_translation.py:109-119
 *   pn2_fps_points         the numpy farthest_point_sample(point_cloud, number) of the data path
 *                                                            provider.py:183-204;
 *                                                            data_utils/ModelNetDataLoader.py:25-46;
 *                                                            point_collect/transformer.py:120-141;
 *                                                            data_build/Cube.py:102-123
 *   pn2_clip_flags / pn2_radius_count_f64 / pn2_compact_rows / pn2_dbscan_labels
 *                          the capture scripts' clip_distance, delet_outlier_radius, cluster_point
 *                                                            point_collect/collect.py:30-102;
 *                                                            camera_test/camera.py:131
 *   pn2_knn_mean_dist_f64 / pn2_stat_outlier_flags
 *                          the capture scripts' delet_outlier_statistical
 *                                                            point_collect/collect.py:80-90
 *   pn2_plane_segment / pn2_plane_refit
 *                          the capture scripts' delete_plane   point_collect/collect.py:6-28
 */
#ifndef PN2_H
#define PN2_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PN2_OK 0
#define PN2_EINVAL (-1)     /* bad argument / shape */
#define PN2_EUNSUPPORTED (-2) /* shape outside what the kernels are built for */
#define PN2_EHIP (-3)       /* HIP runtime error at launch */

#define PN2_ABI_VERSION 19

int pn2_abi_version(void);
const char *pn2_last_error(void);

/* Device error slots: conditions under which the reference raises but a kernel cannot.  The
 * kernels stay in bounds (clamped or NaN outputs, documented per entry point) and OR a bit into
 * the device error slot of the host thread that launched them:
 *   PN2_DEVERR_NO_NEIGHBOUR  a ball-query centroid had no point within the radius (its row is
 *                            padded with N, pointnet2_utils.py:85-89; the reference's next
 *                            index_points raises IndexError); the SA kernels read point 0 there
 *   PN2_DEVERR_INDEX         pn2_index_points_f32 / pn2_group_f32 got an index outside [-N, N)
 *                            (the element is NaN), or pn2_group_backward_f32 did (the position
 *                            contributes nothing)
 * A launch raises into the slot of the device its STREAM belongs to (hipStreamGetDevice; the
 * current device for the null stream), whatever the thread's current device is.
 * pn2_error_slot_set(slot): from now on, launches by the calling thread on the current device
 * raise into `slot` -- two caller-owned, zeroed uint32 DEVICE words ([0] the bits, [1] scratch
 * for the take) that must outlive every launch and captured graph that uses them (a graph
 * raises into the slot of the thread that captured it).  NULL: back to the process-wide
 * default slot, which every thread without a slot of its own shares.
 * pn2_error_slot_take: the calling thread's slot on `stream`'s device, taken -- read and,
 * when `clear` != 0, reset in ONE device atomic, so a bit raised meanwhile is never lost --
 * stream-ordered on `stream`, which it then waits for.
 * pn2_device_errors: the same take after hipDeviceSynchronize (every stream's work done).
 * pn2.check_device_errors() gives each (thread, device) its own slot and raises IndexError. */
#define PN2_DEVERR_NO_NEIGHBOUR 1u
#define PN2_DEVERR_INDEX 2u
int pn2_error_slot_set(uint32_t *slot);
int pn2_error_slot_take(int clear, uint32_t *bits, void *stream);
int pn2_device_errors(int clear, uint32_t *bits);

/* Kernel-selection tuning: int64 parameters of the launch choices (which kernel family, tile
 * widths, block shapes).  The defaults are the measured best (pn2_tuning_default) and the
 * library never reads the environment; tests and A/B tools change them (pn2/tuning.py applies
 * the one PN2_TUNING="key=value,..." variable at load).  Process-wide keys are atomic words:
 * a set on one thread while another launches is safe (the launch sees the old or the new value
 * of each key).  Keys: pn2_tuning_keys() (space-separated). */
int pn2_tuning_get(const char *key, int64_t *value);
int pn2_tuning_set(const char *key, int64_t value);
int pn2_tuning_default(const char *key, int64_t *value);
const char *pn2_tuning_keys(void);
/* pn2_tuning_local(1): this host thread gets its own copy of the keys (taken from the
 * process-wide values at the outermost enter); pn2_tuning_get/set and every launch on this
 * thread then use the copy, other threads are unaffected; pn2_tuning_local(0) leaves (nested
 * enters count).  pn2.pipeline captures its graphs in this mode under its own launch profile. */
int pn2_tuning_local(int enter);

/* Packed point layout used by the ball query: [B][N][cp] float32, cp = pn2_packed_stride(C),
 * holding the C coordinates, then ssq = torch.sum(p**2,-1) computed with the reference's
 * layout-dependent CPU summation order, then zero padding. */
int64_t pn2_packed_stride(int64_t C);

/* Farthest point sampling over points[b, n, c] = pts[b*sb + n*sn + c*sc].
 * start[B] (int64, device) = the reference's torch.randint draw.  Outputs (device):
 *   out_idx    [B,S] int64                      fps indices
 *   out_pts    [B,S,C] float32 contiguous, or NULL   index_points(points, fps_idx)
 *   out_packed [B,S,cp] float32, or NULL         packed centroids (contiguous-layout ssq)
 *   pts_packed [B,N,cp] float32, or NULL         packed input points (input-layout ssq)
 * C <= 64 (else PN2_EUNSUPPORTED: the reference's channel-sum orders are pinned to C = 64);
 * 16 < C <= 64 always runs the streamed kernel (256 threads per cloud; the same workspace rule
 * with the LDS holding up to 40896 distances).  The cloud is register-resident up to N = 16384 for C == 3, 8192 for
 * C == 10, 4096 for other C (past that, up to N = 16384, the channels after xyz are re-read
 * from pts each iteration unless they are constant over the cloud: one-hot), with S <= 8192.
 * Any other N or S runs the streamed kernel: the points re-read every iteration, the running
 * distances in LDS up to N = 40896, past that in a caller workspace of
 * pn2_fps_workspace_bytes(B, N, C, S) bytes (pn2_fps_ws_f32; pn2_fps_f32 passes none and
 * fails with PN2_EINVAL when one is needed). */
int pn2_fps_f32(const float *pts, int64_t B, int64_t N, int64_t C, int64_t sb, int64_t sn,
                int64_t sc, const int64_t *start, int64_t S, int64_t *out_idx, float *out_pts,
                float *out_packed, float *pts_packed, void *stream);
int64_t pn2_fps_workspace_bytes(int64_t B, int64_t N, int64_t C, int64_t S);
int pn2_fps_ws_f32(const float *pts, int64_t B, int64_t N, int64_t C, int64_t sb, int64_t sn,
                   int64_t sc, const int64_t *start, int64_t S, int64_t *out_idx, float *out_pts,
                   float *out_packed, float *pts_packed, void *workspace, int64_t workspace_bytes,
                   void *stream);
/* The same with start_host[B] in HOST memory, as the reference draws it (pointnet2_utils.py:59:
 * torch.randint on the CPU, then .to(device)): read during the call -- the caller may reuse it
 * on return -- and checked (0 <= start < N, else PN2_EINVAL), no host->device copy. */
int pn2_fps_host_ws_f32(const float *pts, int64_t B, int64_t N, int64_t C, int64_t sb, int64_t sn,
                        int64_t sc, const int64_t *start_host, int64_t S, int64_t *out_idx,
                        float *out_pts, float *out_packed, float *pts_packed, void *workspace,
                        int64_t workspace_bytes, void *stream);

/* ---- two consecutive sampling levels in one launch (csrc/fps_body.h fps2_block): level 1
 * samples S1 of the N input points, level 2 samples S2 of level 1's centroids.
 * Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19.
 * What pn2_fps_f32(pts, ..., start1, S1, out_idx1, out_pts1, out_packed1, pts_packed1) followed by
 * pn2_fps_f32(out_pts1 [B,S1,3] contiguous, ..., start2, S2, out_idx2, out_pts2, out_packed2,
 * pts_packed2) write, bit for bit; out_idx1 / out_idx2 required, the others may be NULL.
 * start1[B] in [0, N), start2[B] in [0, S1): int64, device.  One workgroup per cloud; level 2
 * runs on the ceil(S1 / 128) waves it needs, from level 1's records in LDS.
 * pn2_fps2_eligible(N, C, S1, S2): 1 when the shape is taken -- C == 3, N <= 1024, S1 <= 512,
 * S2 <= 8192 and the automatic FPS block choice (tuning fps_threads = fps_ppt = 0, fps_mid = 512)
 * -- else 0, and pn2_fps2_f32 returns PN2_EUNSUPPORTED: the caller runs the two launches. */
int pn2_fps2_eligible(int64_t N, int64_t C, int64_t S1, int64_t S2);
int pn2_fps2_f32(const float *pts, int64_t B, int64_t N, int64_t C, int64_t sb, int64_t sn,
                 int64_t sc, const int64_t *start1, int64_t S1, const int64_t *start2, int64_t S2,
                 int64_t *out_idx1, float *out_pts1, float *out_packed1, float *pts_packed1,
                 int64_t *out_idx2, float *out_pts2, float *out_packed2, float *pts_packed2,
                 void *stream);

/* ---- farthest-point downsampling of raw clouds by the reference's NUMPY rule
 * (provider.py:183-204 and its copies; csrc/fps_points.hip), a ragged batch in one launch.
 * Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19.
 *   pts       [total_rows][ld] rows of `dtype` elements (PN2_DTYPE_F32 / PN2_DTYPE_F64), ld >= C;
 *             cloud b is the rows offsets[b] .. offsets[b+1]-1
 *   offsets   [B+1] int64 row offsets (device), 0 <= offsets[b] < offsets[b+1] <= total_rows,
 *             every cloud of 1 .. max_n rows;  starts [B] int64 (device), the reference's
 *             np.random.randint(0, N) draw of each cloud
 *   out_idx   [B][S] int64: the sampled row of each of the S iterations (S may exceed a cloud's N:
 *             the reference then repeats indices);  out_pts [B][S][C] `dtype`: point_cloud[idx],
 *             all C columns.  Only columns 0..2 are measured.
 * Arithmetic in the input's precision, every operation rounded separately: d_k = x_k - c_k,
 * dist = (d_0*d_0 + d_1*d_1) + d_2*d_2, running distance 1e10 at the start and replaced only when
 * dist < distance, next centroid the FIRST index of the maximum.  Inputs must be finite.
 * One 1024-thread workgroup per cloud.  Two paths, chosen per launch by max_n: the running
 * distances live in LDS while max_n <= (160 KiB - 384) / sizeof(element) (40864 float32, 20432
 * float64 points), else in `workspace`, one element per input row.
 * pn2_fps_points_workspace_bytes(dtype, total_rows, max_n) reports the path: 0 on the LDS path,
 * total_rows * sizeof(element) past it (-1: bad arguments).  The workspace is 8-byte aligned.
 * A cloud whose table entries break the rules above (or whose start is outside [0, N)) is not
 * sampled: its out_idx row is -1, its out_pts rows are not written, PN2_DEVERR_INDEX is raised.
 * B == 0 or S == 0: nothing to do, no launch. */
#define PN2_DTYPE_F32 0
#define PN2_DTYPE_F64 1
int64_t pn2_fps_points_workspace_bytes(int dtype, int64_t total_rows, int64_t max_n);
int pn2_fps_points(const void *pts, int dtype, int64_t B, const int64_t *offsets,
                   const int64_t *starts, int64_t total_rows, int64_t max_n, int64_t C, int64_t ld,
                   int64_t S, int64_t *out_idx, void *out_pts, void *workspace,
                   int64_t workspace_bytes, void *stream);

/* ---- camera-cloud front end: clip_distance, delet_outlier_radius, cluster_point
 * (point_collect/collect.py:30-102 and its copy colledt_data_structure/collect.py;
 * camera_test/camera.py:131; csrc/collect.hip).
 * Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19.
 * A cloud is pts [N][ld] rows of `dtype` elements (PN2_DTYPE_F32 / PN2_DTYPE_F64), 3 <= C <= 64,
 * ld >= C, N <= pn2_collect_max_points() = 2^20 (above: PN2_EUNSUPPORTED; DESIGN.md 4.4 has the
 * arithmetic).  Rows are carried whole; distances use columns 0..2.  Every result is a selection
 * of input rows or an integer, so parity with the rules below is bit for bit.
 *  1 Clip.  Row i is kept iff lo <= p[i][axis] <= hi, compared in float64 (a float32 value widened),
 *    in input order; a NaN fails both tests.
 *  2 Neighbour.  d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in float64 (float32 inputs widened first),
 *    dx = x_i - x_j, every operation rounded once, no contraction.  j is a neighbour of i iff
 *    d2 < r*r, r*r one float64 product.  Every finite point is its own neighbour, and so is each
 *    of its duplicates; a point with a NaN coordinate has no neighbour.
 *  3 Radius filter.  Row i is kept iff its neighbour count, itself included, is > nb_points;
 *    input order.
 *  4 DBSCAN labels.  A point is core iff its neighbour count is >= min_points.  Clusters are the
 *    connected components of the core points under the neighbour relation, numbered 0, 1, ... in
 *    ascending order of their smallest core index.  A non-core point with a core neighbour takes
 *    the smallest label among its core neighbours; every other point is -1.
 *  5 cluster_point: the rows of cluster l in ascending index order, each cluster sampled to the
 *    smallest cluster's size by pn2_fps_points (pn2/collect.py draws the starts).
 *
 * pn2_clip_flags        flags[i] = 1 / 0 by rule 1 (int32 [N], device); 0 <= axis < C.
 * pn2_radius_count_f64  counts[i] = neighbours of i by rule 2 with r = radius (int32 [N]).  Tiled
 *                       brute force: N * N pairs, no atomics, two runs give the same bits.
 * pn2_compact_rows      order-preserving bucket sort of rows by keys[i] (int32 [N], device):
 *                         PN2_COMPACT_FLAG_GT  one bucket (L == 1): the rows with keys[i] > thresh
 *                         PN2_COMPACT_FLAG_LE  one bucket (L == 1): the rows with keys[i] <= thresh
 *                         PN2_COMPACT_LABEL    L buckets: row i to bucket keys[i] when 0 <= keys[i]
 *                                              < L; negative keys are dropped, a key >= L is
 *                                              dropped and raises PN2_DEVERR_INDEX
 *                       out_rows [N][C] `dtype` receives the kept rows (only the first offsets[L] are
 *                       written), bucket after bucket, each in ascending input index; out_src (int32
 *                       [N], or NULL) their input indices; offsets [L+1] int64 (device): bucket b is
 *                       the output rows offsets[b] .. offsets[b+1]-1 -- the table pn2_fps_points
 *                       takes.  Rows move as 16-byte pieces when C and ld are whole multiples of
 *                       16 bytes and both base pointers are 16-byte aligned, else element by element.
 *                       Workspace: pn2_compact_rows_workspace_bytes(N, L) bytes, 16-byte aligned
 *                       (-1: bad arguments, or ceil(N / 256) * L above 2^26 table entries, for
 *                       which the entry returns PN2_EUNSUPPORTED).
 * pn2_dbscan_labels     labels [N] int32 by rule 4 from counts [N] (pn2_radius_count_f64 with
 *                       r = eps) and *nclusters (int64, device) = the number of clusters.  A
 *                       lock-free union-find over the core-core neighbour pairs (32-bit parents, the
 *                       larger root always linked under the smaller by compare-and-swap), then a
 *                       flatten pass, a prefix sum over "is root" and one pass for the non-core
 *                       points.  No host read; two runs give the same bits.  Workspace:
 *                       pn2_dbscan_labels_workspace_bytes(N) bytes, 16-byte aligned.
 * N == 0: PN2_OK, nothing is written, no launch. */
#define PN2_COMPACT_FLAG_GT 0
#define PN2_COMPACT_LABEL 1
#define PN2_COMPACT_FLAG_LE 2
int64_t pn2_collect_max_points(void);
int pn2_clip_flags(const void *pts, int dtype, int64_t N, int64_t C, int64_t ld, int64_t axis,
                   double lo, double hi, int32_t *flags, void *stream);
int pn2_radius_count_f64(const void *pts, int dtype, int64_t N, int64_t C, int64_t ld, double radius,
                         int32_t *counts, void *stream);
int64_t pn2_compact_rows_workspace_bytes(int64_t N, int64_t L);
int pn2_compact_rows(const void *pts, int dtype, int64_t N, int64_t C, int64_t ld,
                     const int32_t *keys, int mode, int64_t thresh, int64_t L, void *out_rows,
                     int32_t *out_src, int64_t *offsets, void *workspace, int64_t workspace_bytes,
                     void *stream);
int64_t pn2_dbscan_labels_workspace_bytes(int64_t N);
int pn2_dbscan_labels(const void *pts, int dtype, int64_t N, int64_t C, int64_t ld, double eps,
                      int64_t min_points, const int32_t *counts, int32_t *labels, int64_t *nclusters,
                      void *workspace, int64_t workspace_bytes, void *stream);

/* ---- statistical outlier removal: delet_outlier_statistical (point_collect/collect.py:80-90;
 * csrc/knn.hip), Open3D's RemoveStatisticalOutliers with its kd-tree replaced by exact arithmetic.
 * Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19.
 * The cloud is the camera-cloud front end's (above): pts [N][ld], 3 <= C <= 64, float32 or float64,
 * N <= pn2_collect_max_points().  k = nb_neighbors, 1 <= k <= pn2_knn_max_k() = 256.
 *  S1 Candidates.  A row is finite when its three coordinates are finite.  Only finite rows are
 *     candidates and queries.  F = the number of finite rows, k_eff = min(k, F).
 *  S2 Distance.  d2(i,j) is rule 2's: ((dx*dx) + (dy*dy)) + (dz*dz) in float64 (float32 inputs
 *     widened first), every operation rounded once, no contraction.
 *  S3 Mean distance.  For a finite row i: the k_eff smallest d2(i,j) over all finite j (i itself
 *     included, d2 = 0), sorted ascending; the correctly rounded sqrt of each; added in that order as
 *     one float64 chain from 0.0; divided once by (double)k_eff.  Ties at the k-th place carry equal
 *     values, so the bits do not depend on which tied row is taken.  mean[i] = -1.0 for a non-finite
 *     row.
 *  S4 Cloud statistics.  valid = F.  cloud_mean = (sum of mean[i], i ascending, only the terms with
 *     mean[i] > 0) / valid.  sq_sum = sum over i ascending of (mean[i] - cloud_mean) * (mean[i] -
 *     cloud_mean) where mean[i] > 0, else of 0.  std = sqrt(sq_sum / (valid - 1)).  threshold =
 *     cloud_mean + std_ratio * std.  Each sum is one float64 chain in index order; every operation
 *     is rounded once.  valid == 1 gives 0/0 = NaN and nothing is kept: IEEE, no special case.
 *  S5 Selection.  Row i is kept iff mean[i] > 0 && mean[i] < threshold, in input order.  A row whose
 *     k_eff nearest rows are all its duplicates has mean 0 and is dropped, as Open3D drops it.
 *     F == 0 or N == 0: nothing is kept.
 *
 * pn2_knn_mean_dist_f64   mean [N] float64 (device) by S1-S3.  Brute force over N * N pairs: the
 *                         candidates staged in LDS tiles, a wave per few queries, a ballot against
 *                         the query's current k-th value, the survivors bitonic-sorted in LDS.  No
 *                         atomics: two runs give the same bits.  k < 1: PN2_EINVAL; k >
 *                         pn2_knn_max_k(): PN2_EUNSUPPORTED.  Workspace (the float64 coordinates):
 *                         pn2_knn_mean_dist_workspace_bytes(N, k) bytes, 16-byte aligned (-1: bad
 *                         arguments).
 * pn2_stat_outlier_flags  one launch of one workgroup, no host read: stats [4] float64 (device) =
 *                         {cloud_mean, std, threshold, (double)valid} by S4 and flags[i] = 1 / 0
 *                         (int32 [N]) by S5 from mean [N].  std_ratio <= 0: PN2_EINVAL.  The kept
 *                         rows are pn2_compact_rows(flags, PN2_COMPACT_FLAG_GT, thresh = 0).
 * N == 0: PN2_OK, nothing is written, no launch. */
int64_t pn2_knn_max_k(void);
int64_t pn2_knn_mean_dist_workspace_bytes(int64_t N, int64_t k);
int pn2_knn_mean_dist_f64(const void *pts, int dtype, int64_t N, int64_t C, int64_t ld, int64_t k,
                          double *mean, void *workspace, int64_t workspace_bytes, void *stream);
int pn2_stat_outlier_flags(const double *mean, int64_t N, double std_ratio, int32_t *flags,
                           double *stats, void *stream);

/* ---- plane segmentation: delete_plane (point_collect/collect.py:6-28; csrc/plane.hip), Open3D's
 * segment_plane (RANSAC) with the draws made an input and everything after them exact arithmetic.
 * Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19.
 * The cloud is the camera-cloud front end's (above): pts [N][ld], 3 <= C <= 64, float32 or float64,
 * N <= pn2_collect_max_points().  Only columns 0..2 are measured; float32 inputs are widened to
 * float64 first.  Every operation below is one float64 operation rounded once, no contraction;
 * sqrt and / are correctly rounded.  M = num_iterations, 1 <= M <= pn2_plane_max_iterations() = 4096;
 * n = ransac_n, 3 <= n <= pn2_plane_max_ransac_n() = 64; thr = distance_threshold, finite and > 0.
 * This is Open3D's published structure (GetPlaneFromPoints, ComputeTrianglePlane, the
 * count-then-error comparison, the refit over the inliers) restated.  The association of the dot
 * products, the error term (the sum of the inliers' distances) and its order, the draws and the
 * absence of the early exit are this project's choices, and none of it has been checked against an
 * Open3D build.
 *  P1 Samples.  samples [M][n] int32 (device), every entry in [0, N): an INPUT of the kernels.
 *     pn2.collect draws them with one call, np.random.randint(0, N, size=(M, n)), from numpy's
 *     global generator, unless the caller passes samples=.  A row may repeat an index: a repeated
 *     point counts that many times in P2.  A row with an entry outside [0, N) is skipped like a
 *     zero plane and raises PN2_DEVERR_INDEX.
 *  P2 Hypothesis, n > 3 (GetPlaneFromPoints).  The row's points in row order:
 *     centroid_k = (chain sum of p_k from 0.0) / (double)n; r = p - centroid; the six sums xx, xy,
 *     xz, yy, yz, zz of r_i * r_j, each one chain from 0.0 in row order.
 *       det_x = yy*zz - yz*yz    det_y = xx*zz - xz*xz    det_z = xx*yy - xy*xy
 *       det_x > det_y && det_x > det_z:  abc = (det_x, xz*yz - xy*zz, xy*yz - xz*yy)
 *       else det_y > det_z:              abc = (xz*yz - xy*zz, det_y, xy*xz - yz*xx)
 *       else:                            abc = (xy*yz - xz*yy, xy*xz - yz*xx, det_z)
 *     norm = sqrt((a*a + b*b) + c*c).  norm == 0 gives the zero plane (0, 0, 0, 0).  Otherwise
 *     abc = abc / norm (three divisions) and d = -((a*cx + b*cy) + c*cz).
 *  P3 Hypothesis, n == 3 (ComputeTrianglePlane).  e0 = p1 - p0, e1 = p2 - p0,
 *     abc = (e0y*e1z - e0z*e1y, e0z*e1x - e0x*e1z, e0x*e1y - e0y*e1x); the norm, the zero test and
 *     the normalisation as in P2; d = -((a*p0x + b*p0y) + c*p0z).
 *  P4 Score.  dist_i = |((a*x_i + b*y_i) + c*z_i) + d|.  Point i is an inlier iff dist_i < thr; a NaN
 *     fails, so a non-finite row is never an inlier.  count = the number of inliers.  err = the sum
 *     of the inliers' dist_i in this order: the rows are cut into chunks of PN2_PLANE_CHUNK = 1024
 *     consecutive indices; within a chunk one chain from 0.0 in ascending index; the chunk sums
 *     added in ascending chunk order as one chain from 0.0.  A zero plane (P2/P3) is not scored:
 *     count 0, err 0.0.
 *  P5 Best.  Start from (count 0, err 0.0, index -1, plane 0).  Walk the hypotheses in ascending m:
 *     hypothesis m replaces the best iff count_m > count || (count_m == count && err_m < err).
 *     Among full ties the lowest index wins, and a plane with a NaN coefficient (count 0) never
 *     wins.  This is Open3D's loop without its probabilistic early exit: every hypothesis is
 *     scored.  If the index stays -1, nothing is an inlier (Open3D's all-zero model would call every
 *     point an inlier: a stated deviation).
 *  P6 Inliers.  flags[i] = 1 iff dist_i < thr under the best plane, else 0: the set Open3D returns.
 *  P7 Refit (the model Open3D returns).  GetPlaneFromPoints (P2's formulas) over the flagged rows
 *     (flags[i] != 0): first the centroid, then the six second moments, each sum in P4's chunked
 *     order, n = the number of flagged rows.  With no flagged row the plane is zero.  P6 never flags
 *     a non-finite row; a caller's flag on one makes the sums, and so the plane, NaN.
 *
 * pn2_plane_segment  P1-P6 as four launches on `stream`, no host read: fit (one thread per
 *                    hypothesis), score (a workgroup per 1024-row chunk and 256 hypotheses: the
 *                    chunk in LDS, a hypothesis' plane in registers, each thread its own count and
 *                    err chain), select (chunk partials added in chunk order, then the best by the
 *                    total key count desc, err asc, index asc), flag.  No atomics on floats: two
 *                    runs give the same bits.  flags [N] int32; result [8] float64 (device) =
 *                    {a, b, c, d, (double)best_index, (double)count, err, 0} of P5.  out_planes
 *                    [M][4] float64, out_count [M] int32, out_err [M] float64 (device; each may be
 *                    NULL): every hypothesis' plane, count and err; a skipped hypothesis writes a
 *                    zero plane, count 0 and err 0.0.  n < 3, M < 1 or a threshold that is not
 *                    finite and > 0: PN2_EINVAL; n or M above its cap: PN2_EUNSUPPORTED.
 *                    Workspace (the float64 coordinates, the hypotheses and the per-chunk x
 *                    per-hypothesis partials (int32 count, float64 err)):
 *                    pn2_plane_segment_workspace_bytes(N, M) bytes, 16-byte aligned (-1: bad
 *                    arguments).
 * pn2_plane_score    for measurement: the score launch of pn2_plane_segment alone, on a workspace
 *                    that a pn2_plane_segment call with the same N and M has filled (it reads the
 *                    coordinates and hypotheses there and rewrites the partials with the same bits
 *                    when the threshold is the same).  Checks as pn2_plane_segment's.
 * pn2_plane_refit    plane [4] float64 (device) by P7 from flags [N] int32: two rounds (centroid,
 *                    moments) of a chunk-partials launch and a one-wave finishing launch.
 *                    Workspace: pn2_plane_refit_workspace_bytes(N) bytes, 16-byte aligned.
 * The rows that are not inliers are pn2_compact_rows(flags, PN2_COMPACT_FLAG_LE, thresh = 0).
 * N == 0: PN2_OK, nothing is written, no launch. */
#define PN2_PLANE_CHUNK 1024
int64_t pn2_plane_max_ransac_n(void);
int64_t pn2_plane_max_iterations(void);
int64_t pn2_plane_segment_workspace_bytes(int64_t N, int64_t M);
int pn2_plane_segment(const void *pts, int dtype, int64_t N, int64_t C, int64_t ld,
                      const int32_t *samples, int64_t M, int64_t n, double distance_threshold,
                      int32_t *flags, double *result, double *out_planes, int32_t *out_count,
                      double *out_err, void *workspace, int64_t workspace_bytes, void *stream);
int pn2_plane_score(int64_t N, int64_t M, double distance_threshold, void *workspace,
                    int64_t workspace_bytes, void *stream);
int64_t pn2_plane_refit_workspace_bytes(int64_t N);
int pn2_plane_refit(const void *pts, int dtype, int64_t N, int64_t C, int64_t ld,
                    const int32_t *flags, double *plane, void *workspace, int64_t workspace_bytes,
                    void *stream);

/* Pack a [B,N,C] strided view into [B,N,cp] with its ssq (see above).  C <= 64, as for the
 * ball query and square_distance below (else PN2_EUNSUPPORTED). */
int pn2_pack_points_f32(const float *pts, int64_t B, int64_t N, int64_t C, int64_t sb,
                        int64_t sn, int64_t sc, float *packed, void *stream);

/* query_ball_point: for every centroid, the first K point indices (ascending) whose
 * square_distance is not > (float)(radius*radius), padded with the first hit (N if none).
 * pts_packed [B,N,cp], ctr_packed [B,S,cp] from pn2_pack_points_f32 / pn2_fps_f32.
 * out_idx [B,S,K] int64.  Any 1 <= K <= N (rows that fit a 96 KB LDS buffer are built there and
 * written out whole; longer ones are written in place).  K > N is rejected with PN2_EINVAL
 * (the reference raises IndexError).  16 < C <= 64: a register-light kernel that walks the
 * records in index order per centroid (same results; not tuned -- no BASELINE config has it). */
int pn2_ball_query_f32(const float *pts_packed, const float *ctr_packed, int64_t B, int64_t N,
                       int64_t S, int64_t C, double radius, int64_t K, int64_t *out_idx,
                       void *stream);
/* The same, also writing out_cnt [B,S] int32 (or NULL): the number of distinct neighbours of
 * each centroid, min(hits, K) -- out_idx entries past it repeat entry 0.  Passed to the SA MLP
 * (pn2_sa_src.cnt) it lets the chain compute only those rows (the max over a group does not
 * change without repeats). */
int pn2_ball_query_cnt_f32(const float *pts_packed, const float *ctr_packed, int64_t B,
                           int64_t N, int64_t S, int64_t C, double radius, int64_t K,
                           int64_t *out_idx, int32_t *out_cnt, void *stream);
/* The same lists as int32 (half the bytes; the SA layers' fused path reads them through
 * pn2_sa_src.idx32).  Entries, padding and counts as pn2_ball_query_cnt_f32. */
int pn2_ball_query_i32(const float *pts_packed, const float *ctr_packed, int64_t B, int64_t N,
                       int64_t S, int64_t C, double radius, int64_t K, int32_t *out_idx,
                       int32_t *out_cnt, void *stream);
/* nr (1..3) radii of one centroid set in one launch -- the scales of an MSG layer
 * (pointnet2_utils.py:197-203 calls query_ball_point once per radius): each pair's distance
 * computed once and tested against every radius; out_idx[r] [B,S,K[r]] int32 and out_cnt[r]
 * [B,S] (or out_cnt / out_cnt[r] NULL) exactly as nr pn2_ball_query_i32 calls would write them. */
int pn2_ball_query_multi_i32(const float *pts_packed, const float *ctr_packed, int64_t B,
                             int64_t N, int64_t S, int64_t C, int nr, const double *radii,
                             const int64_t *K, int32_t *const *out_idx, int32_t *const *out_cnt,
                             void *stream);

/* square_distance(src, dst) -> out [B,S,N] float32 from packed records of src [B,S,cp] and
 * dst [B,N,cp] (same float32 recipe as the ball query). */
int pn2_square_distance_f32(const float *src_packed, const float *dst_packed, int64_t B,
                            int64_t S, int64_t N, int64_t C, float *out, void *stream);

/* out[b, m, :] = pts[b, idx[b*M + m], :] ; out contiguous [B,M,C]. idx int64 [B,M]. */
int pn2_index_points_f32(const float *pts, int64_t B, int64_t N, int64_t C, int64_t sb,
                         int64_t sn, int64_t sc, const int64_t *idx, int64_t M, float *out,
                         void *stream);

/* Grouping: out[b,s,k,:] (contiguous [B,S,K,C+D]) =
 *   feature_first == 0 : [pts[b,idx]-ctr[b,s], feat[b,idx]]   (sample_and_group, SSG)
 *   feature_first == 1 : [feat[b,idx], pts[b,idx]-ctr[b,s]]   (PointNetSetAbstractionMsg)
 * feat may be NULL (D = 0).  ctr is contiguous [B,S,C]; feat element (b,n,d) at
 * feat[b*fb + n*fn + d*fd]. */
int pn2_group_f32(const float *pts, int64_t B, int64_t N, int64_t C, int64_t sb, int64_t sn,
                  int64_t sc, const float *feat, int64_t D, int64_t fb, int64_t fn, int64_t fd,
                  const float *ctr, int64_t S, const int64_t *idx, int64_t K, int feature_first,
                  float *out, void *stream);

/* ---- backward of the grouping for the features (csrc/group.hip): every grouped row's feature
 * gradient summed back into its source point, in a fixed order and without float atomics.
 * Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19.
 *   dgrouped  [B,S,K,.] float32: row (b,s,k) starts at dgrouped[((b*S + s)*K + k) * row_stride],
 *             its D feature columns at `offset` (0 for feature_first rows, C otherwise),
 *             offset + D <= row_stride; read in place, 16-byte loads when D, offset, row_stride
 *             and both bases allow them
 *   idx       [B,S,K] int64 (PN2_INDEX_I64) or int32 (PN2_INDEX_I32), element (b,s,k) at
 *             idx[b*ib + s*is + k*ik]
 *   dfeat     [B,N,D] float32 contiguous, FULLY written: a point no position names gets +0.0
 * The sum rule: dfeat[b,n,d] is the float32 sum of dgrouped[b,s,k,offset+d] over the positions
 * with idx[b,s,k] == n, taken in ascending (s,k) order from +0.0f, one rounding per add -- what
 * np.add.at and torch's CPU index_add_ compute, bit for bit, and the same bits on every run.
 * Indices as pn2_group_f32: [-N, 0) counts from the end; outside [-N, N) the position
 * contributes nothing and PN2_DEVERR_INDEX is raised.
 * workspace: pn2_group_backward_workspace_bytes(B, N, S, K) bytes (-1: bad arguments), 4-byte
 * aligned; the table of each point's positions is built there on every call.  S*K, B*N and D
 * must each be below 2^31.  B == 0: nothing to do, no launch. */
#define PN2_INDEX_I64 0
#define PN2_INDEX_I32 1
int64_t pn2_group_backward_workspace_bytes(int64_t B, int64_t N, int64_t S, int64_t K);
int pn2_group_backward_f32(const float *dgrouped, int64_t row_stride, int64_t offset,
                           const void *idx, int idx_dtype, int64_t ib, int64_t is, int64_t ik,
                           int64_t B, int64_t N, int64_t S, int64_t K, int64_t D, float *dfeat,
                           void *workspace, int64_t workspace_bytes, void *stream);

/* ---- the three matrix products of a shared-MLP layer's training step (csrc/train_gemm.hip),
 * every sum in a fixed, documented order: no float atomics, no workgroup waits on another.
 * Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19.
 * All operands float32 row-major with a leading dimension (>= the matrix width), read and
 * written in place through it; no load ever passes the end of a row, 16-byte loads only where
 * base and leading dimension allow them.  Arithmetic: each operand value in three bf16 planes,
 * six v_mfma_f32_32x32x16_bf16 per product step (csrc/split_bf16.h): fp32-GEMM accuracy.
 *   pn2_gemm_nt_f32  C[M,N] = A[M,K] B[N,K]^T (+ bias[N]; bias may be NULL)    Y  = X W^T + b
 *   pn2_gemm_nn_f32  C[M,N] = A[M,K] B[K,N]   (B as stored: no transpose copy) dX = dY W
 *   pn2_gemm_tn_f32  C[N,K] = A[M,N]^T B[M,K] (the sum over the M rows)        dW = dY^T X
 * Order of nt and nn: an element's accumulator starts at +0 and takes the reduction dimension
 * in ascending 16-wide steps (zero-padded past its end); the bias is added once, at the end.
 * ROW INDEPENDENCE of nt and nn: row r of C is a function of row r of A, of B and of the bias
 * only -- not of M, not of the row's position: the reduction is never split by anything that
 * depends on M.
 * THE ORDER RULE of tn:
 *   1. the rows are cut into slabs of R = pn2_gemm_tn_slab_rows() rows (a compile-time constant,
 *      a multiple of 32): slab j holds rows [j*R, min((j+1)*R, M));
 *   2. slab j's partial P_j is a float32 [N,K] matrix that depends only on that slab's rows
 *      -- not on j, M, the device's CU count or what else runs: it is, bit for bit, what this
 *      entry returns when called on that slab alone (inside a slab: ascending 16-row steps
 *      from +0, fixed);
 *   3. C = float32(sum_j double(P_j)), added in ascending j from +0.0 in float64, rounded once.
 *   One launch writes the partials to `workspace`, a second one reduces them; M <= R takes the
 *   same two steps.  workspace: pn2_gemm_tn_workspace_bytes(M, N, K) = ceil(M/R) * N * K * 4
 *   bytes exactly (-1: bad arguments), 4-byte aligned.
 * Limits: 1 <= N, K <= 4096 (above: PN2_EUNSUPPORTED); M >= 0; M == 0 returns PN2_OK, launches
 * nothing and writes nothing (also for tn, whose C would be all zero).  Violations are reported
 * before any device call.  Non-finite inputs: the outputs that depend on one are non-finite
 * (Inf or NaN: the split of an Inf has a NaN residual), all others are unaffected. */
int pn2_gemm_nt_f32(const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias,
                    float *C, int64_t ldc, int64_t M, int64_t N, int64_t K, void *stream);
int pn2_gemm_nn_f32(const float *A, int64_t lda, const float *B, int64_t ldb, float *C,
                    int64_t ldc, int64_t M, int64_t N, int64_t K, void *stream);
int64_t pn2_gemm_tn_slab_rows(void);
int64_t pn2_gemm_tn_workspace_bytes(int64_t M, int64_t N, int64_t K);
int pn2_gemm_tn_f32(const float *A, int64_t lda, const float *B, int64_t ldb, float *C,
                    int64_t ldc, int64_t M, int64_t N, int64_t K, void *workspace,
                    int64_t workspace_bytes, void *stream);

/* ---- a heads' fully connected layer under autograd, one launch each way (csrc/fc_train.hip):
 * Linear + BatchNorm1d (batch or running statistics) + ReLU forward, and its backward up to dY,
 * dW and the parameter gradients, for batches that fit one workgroup.
 * Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19.
 * Reference: fc1/bn1/relu, fc2/bn2/relu, fc3 under the training loops' autograd,
 * model/pointnet2_cls_ssg.py:31-36, rotation_ssg.py:33-37, translation_ssg.py:23-26,
 * pointnet_utils.py:33-40.
 * All matrices float32 row-major with a leading dimension (>= the width), read and written in
 * place through it; 16-byte loads only where base and leading dimension allow, no load past an
 * edge.  Plain float32 FMA arithmetic.  B <= pn2_fc_train_max_rows() (a compile-time constant,
 * >= 64); a workgroup owns 4 output columns and all B rows of them.
 *
 * pn2_fc_bn_forward_f32: X [B][K], W [N][K], bias [N] -> Y [B][N] = X W^T + bias (always
 *   written: the backward reads it), A [B][N] = act(bn(Y)), flags PN2_LAYER_*:
 *   gamma != NULL, no PN2_LAYER_FROZEN_STATS: batch statistics.  Per column s = sum_r Y,
 *     q = sum_r Y*Y in float64, mean = s/B, var = max(q/B - mean^2, 0), invstd =
 *     1/sqrt(var + eps); stats = [float32(mean) | float32(invstd)] (2N floats);
 *     A = act((Y - mean)*invstd*gamma + beta) with the rounded statistics (float32 operations,
 *     each rounded on its own).  momentum > 0: running_mean/var = (1-momentum)*old + momentum*
 *     (mean, var*B/(B-1)) in float64 (torch's rule; pn2_bn_train_stats_f32's); momentum <= 0:
 *     the running statistics are neither read nor written and may be NULL.  B == 1: PN2_EINVAL.
 *   gamma != NULL, PN2_LAYER_FROZEN_STATS: mean = running_mean, invstd = float32(1/sqrt(
 *     double(running_var) + eps)), both only read; stats receives them.
 *   gamma == NULL: no BatchNorm, A = act(Y); stats, beta and the running statistics are not
 *     touched and may be NULL.
 *   act is the ReLU (x > 0 ? x : 0), the identity with PN2_LAYER_NO_RELU.
 * pn2_fc_bn_backward_f32: dA [B][N], the forward's Y, X and stats (and gamma, beta: the same
 *   pointers-or-NULL and the same flags as the forward) ->
 *     dXn = dA * [A > 0], A recomputed from Y and stats by the forward's expression (dA itself
 *       with PN2_LAYER_NO_RELU);
 *     dbeta[N] = float32(sum_r dXn), dgamma[N] = float32(sum_r dXn * xhat), float64 sums of
 *       float64 products, xhat = (Y - mean)*invstd in float64 inside the sum;
 *     dY [B][N] = gamma*invstd*(dXn - dbeta/B - xhat*dgamma/B) (batch statistics; float32,
 *       the two means rounded to float32 first), gamma*invstd*dXn (frozen), dXn (no BN);
 *     dbias[N] = float32(sum_r double(dY));  dW [N][K] = sum_r dY[r][n] * X[r][k].
 *   dX is not computed here: it is pn2_gemm_nn_f32(dY, W).  dgamma / dbeta may be NULL (and
 *   are not written) when gamma is NULL.
 * THE ORDER RULES:
 *   1. An element of Y is one chain acc = fma(X[r][k], W[n][k], acc) (a single rounding per
 *      step) over k = 0, 1, .. K-1 from +0, then one float32 add of bias[n].  The order
 *      depends on K alone: not on B, N, the row's or column's position or a leading dimension.
 *      ROW INDEPENDENCE: row r of Y is a function of row r of X, of W and of the bias only.
 *   2. Every column sum over the rows (s, q, dbeta, dgamma, dbias) is a float64 sum in
 *      ascending row order r = 0 .. B-1 from +0.0.  An element of dW is acc = fma(dY[r][n],
 *      X[r][k], acc) in float32 over r = 0 .. B-1 from +0.0f: an fma, one rounding per step
 *      (the unit is compiled without contraction; an fma is only where the source asks).
 *   3. No float atomics.
 *   4. No workgroup waits for, or reads, another's result; no workspace.
 * Errors, before any device call: PN2_EINVAL for B < 1, N < 1, K < 1, a leading dimension below
 * its width, a NULL required pointer, gamma without beta / stats (/ dgamma / dbeta), unknown
 * flags, batch statistics with B == 1; PN2_EUNSUPPORTED for B > pn2_fc_train_max_rows(). */
int64_t pn2_fc_train_max_rows(void);
int pn2_fc_bn_forward_f32(const float *X, int64_t ldx, const float *W, int64_t ldw, const float *bias,
                          int64_t B, int64_t N, int64_t K, double eps, double momentum,
                          float *running_mean, float *running_var,
                          const float *gamma, const float *beta,
                          float *Y, int64_t ldy, float *A, int64_t lda,
                          float *stats /* [mean | invstd], 2N */, int flags, void *stream);
int pn2_fc_bn_backward_f32(const float *dA, int64_t ldd, const float *Y, int64_t ldy,
                           const float *X, int64_t ldx, const float *stats,
                           const float *gamma, const float *beta,
                           int64_t B, int64_t N, int64_t K,
                           float *dY, int64_t ldyy, float *dW, int64_t ldw, float *dbias,
                           float *dgamma, float *dbeta, int flags, void *stream);

/* ---- the same layer for any number of rows (csrc/fc_train.hip: the entries above are the
 * one-slab instantiation of its forward / backward kernel template, these the slab loop):
 * pn2_fc_bn_forward_rows_f32 / pn2_fc_bn_backward_rows_f32 take the argument lists of
 * pn2_fc_bn_forward_f32 / pn2_fc_bn_backward_f32, name for name, and serve 1 <= B <= 2^30.
 * Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19.
 * The whole contract above applies: the meaning of every output and flag, THE ORDER RULES 1-4
 * as written (none of them names a row limit), the leading dimensions, 16-byte loads only where
 * base and leading dimension allow, no load past an edge, and the same PN2_EINVAL cases before
 * any device call (batch statistics with B == 1 included).  What the rules mean above 64 rows:
 *   1. a row of Y is the same fma chain over k whatever B is: rows of Y equal, bit for bit,
 *      what either forward entry gives for any subset of the rows of X;
 *   2. s, q, dbeta, dgamma and dbias stay ONE float64 chain over r = 0 .. B-1 per column, an
 *      element of dW ONE float32 fma chain over r = 0 .. B-1: a column's rows are never split
 *      over lanes or workgroups and no partial sums are combined.  A workgroup owns 4 columns
 *      and walks all B rows of them in slabs of pn2_fc_train_max_rows() rows, carrying its
 *      accumulators from slab to slab in row order -- so the launch has ceil(N/4) workgroups
 *      whatever B is, and its time grows with B;
 *   3., 4. no float atomics, no wait for another workgroup, no workspace.
 * For B <= pn2_fc_train_max_rows() the results are bit for bit those of the entries above (one
 * source for both: every expression and every order of summation is written once).
 * With batch statistics the forward reads its own Y back to write A: Y and A must not overlap
 * (as above).  PN2_EUNSUPPORTED for B > 2^30 (the kernels count rows in an int32). */
int pn2_fc_bn_forward_rows_f32(const float *X, int64_t ldx, const float *W, int64_t ldw, const float *bias,
                               int64_t B, int64_t N, int64_t K, double eps, double momentum,
                               float *running_mean, float *running_var,
                               const float *gamma, const float *beta,
                               float *Y, int64_t ldy, float *A, int64_t lda,
                               float *stats /* [mean | invstd], 2N */, int flags, void *stream);
int pn2_fc_bn_backward_rows_f32(const float *dA, int64_t ldd, const float *Y, int64_t ldy,
                                const float *X, int64_t ldx, const float *stats,
                                const float *gamma, const float *beta,
                                int64_t B, int64_t N, int64_t K,
                                float *dY, int64_t ldyy, float *dW, int64_t ldw, float *dbias,
                                float *dgamma, float *dbeta, int flags, void *stream);

/* ---- the reductions after the heads' last layer, and the loops' metrics (csrc/loss.hip):
 * log_softmax under autograd, the four criteria of the get_loss classes, and the test loops'
 * per-class bookkeeping accumulated on the device.
 * Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19.
 * Reference: the get_loss classes of model/pointnet2_cls_ssg.py:40-47 (F.nll_loss),
 * rotation_ssg.py:40-50 (nn.MSELoss / nn.L1Loss, reduction 'mean' or 'sum') and
 * sign_ssg.py:38-45 (nn.BCELoss); F.log_softmax at pointnet2_cls_ssg.py:36; the bookkeeping of
 * train_classification.py:121-122, 144-150, train_rotation.py:126-127, 157-163 and
 * train_sign.py:148-153.
 * float32 matrices are row-major with a leading dimension (>= the width), read and written in
 * place through it; targets are int64 where the reference's are.  Every call is async on the
 * caller's stream and uses no workspace.  The unit is compiled without contraction: every
 * operation below rounds on its own; exp and log are float64 library functions, everything else
 * is an IEEE operation.
 *
 * pn2_log_softmax_rows_f32: X [B][K] -> Y [B][K], 1 <= K <= 1024, 1 <= B <= 2^30.  Per row,
 *   independent of every other row and of B:
 *     m = max_j x_j;  s = sum_j exp(double(x_j) - double(m)) in ascending j from +0.0, in
 *     float64;  y_j = float32((double(x_j) - double(m)) - log(s)).
 * pn2_log_softmax_rows_backward_f32: dY, the forward's Y -> dX:
 *     g = sum_j double(dy_j) in ascending j from +0.0;
 *     dx_j = float32(double(dy_j) - exp(double(y_j)) * g).
 *
 * pn2_criterion_forward_f32: P [B][K] float32, kind PN2_LOSS_*, reduction PN2_REDUCE_* -> one
 *   float32 at `loss`.  target: int64 [B] for PN2_LOSS_NLL (ldt is not read), float32 [B][K]
 *   (leading dimension ldt) otherwise.  Element terms, in float64 from the float32 inputs:
 *     NLL  -P[b][t_b]                                          (one term per row)
 *     MSE  d*d,  d = double(p) - double(t)
 *     L1   |d|
 *     BCE  -(t*max(log(p), -100) + (1-t)*max(log(1-p), -100))   (torch's clamp; p is not
 *          checked to lie in [0, 1]: outside it the term is NaN)
 *   THE ORDER RULE: the loss is ONE float64 chain acc = acc + term over the terms in row-major
 *   order (b ascending, then j ascending) from +0.0.  PN2_REDUCE_SUM rounds the chain to
 *   float32 once; PN2_REDUCE_MEAN divides it in float64 by the term count (B for NLL, B*K
 *   otherwise) and rounds once.  No float atomics; no partial sums exist, so none are combined:
 *   the launch is one workgroup whose threads compute the terms side by side, and only the adds
 *   are ordered.  The serial chain is an accepted cost (B*K is a few thousand for every
 *   reference shape), as in the slab kernels above.
 * pn2_criterion_backward_f32: the same arguments, g a DEVICE pointer to the upstream float32
 *   scalar -> dP [B][K] = float32((double(g)*c)*term'), c = 1 (sum) or 1.0/count (mean) in
 *   float64, the products in that order in float64, rounded once.  term':
 *     NLL  -1 at the target column, 0 elsewhere; the whole row is written
 *     MSE  2*d
 *     L1   sign(d): 1, -1, or 0 at d == 0
 *     BCE  (p - t) / max((1 - p)*p, 1e-12)
 *   An NLL target outside [0, K): the forward's term is NaN (the loss is NaN), the backward
 *   writes +0 to the whole row; nothing is read or written with that index.
 *
 * pn2_meter_update: ONE launch per batch adds that batch to device-resident float64 state:
 *   acc [num_category][W], one `invalid` count, and the batch's record at records[slot*RW ..]
 *   (records holds `slots` records; the host passes the index).  Kinds:
 *     PN2_METER_CLS   pred, target int64 [B] (ldp, ldt, label not read; the category of a row
 *       is its target), W = 2, RW = 1.  For every category c present in the batch:
 *       acc[c][0] += double(correct_c)/double(count_c), acc[c][1] += 1.
 *       record = double(correct)/double(B).
 *     PN2_METER_SIGN  pred, target float32 [B] with strides ldp, ldt, label int64 [B], W = 2,
 *       RW = 1: acc[c][0] += correct_c, acc[c][1] += count_c; record = correct/B.  A row is
 *       correct when pred == target as floats.
 *     PN2_METER_POSE  pred, target float32 [B][D], label int64 [B], W = 1 + D, RW = D:
 *       a = |p - t|, one float32 subtraction.  Per category present and per axis: the float64
 *       chain of a over that category's rows in row order from +0.0, divided by the count,
 *       rounded to float32, then added to acc[c][1+axis]; acc[c][0] += 1.  record[axis] = the
 *       same float32 mean over all B rows.
 *   D is 1 for CLS and SIGN.  A category absent from the batch keeps its row's bits.  A label
 *   outside [0, num_category) is skipped -- nothing is indexed with it -- and counted in
 *   invalid[0]; the records count every row.  One workgroup: a thread per (category, column),
 *   per record column and for the invalid count walks the rows in order.  Two updates of one
 *   state must be ordered on one stream.
 *
 * Errors, before any device call: PN2_EINVAL for B < 1, K < 1 (D < 1, num_category < 1), a
 * leading dimension below its width, a NULL required pointer, an unknown kind or reduction, D
 * != 1 for CLS / SIGN, a slot outside [0, slots); PN2_EUNSUPPORTED for B > 2^30 (rows are
 * counted in an int32), log_softmax with K > 1024, a criterion with K > 2^30, a meter with
 * D > 16 or num_category > 4096. */
#define PN2_LOSS_NLL 0
#define PN2_LOSS_MSE 1
#define PN2_LOSS_L1 2
#define PN2_LOSS_BCE 3
#define PN2_REDUCE_MEAN 0
#define PN2_REDUCE_SUM 1
#define PN2_METER_CLS 0
#define PN2_METER_SIGN 1
#define PN2_METER_POSE 2
int pn2_log_softmax_rows_f32(const float *X, int64_t ldx, float *Y, int64_t ldy, int64_t B, int64_t K,
                             void *stream);
int pn2_log_softmax_rows_backward_f32(const float *dY, int64_t ldd, const float *Y, int64_t ldy, float *dX,
                                      int64_t ldx, int64_t B, int64_t K, void *stream);
int pn2_criterion_forward_f32(int kind, int reduction, const float *P, int64_t ldp, const void *target,
                              int64_t ldt, int64_t B, int64_t K, float *loss, void *stream);
int pn2_criterion_backward_f32(int kind, int reduction, const float *P, int64_t ldp, const void *target,
                               int64_t ldt, const float *g, int64_t B, int64_t K, float *dP, int64_t ldd,
                               void *stream);
int pn2_meter_update(int kind, const void *pred, int64_t ldp, const void *target, int64_t ldt,
                     const int64_t *label, int64_t B, int64_t D, int64_t num_category, double *acc,
                     double *invalid, double *records, int64_t slot, int64_t slots, void *stream);

/* ---- the PointNet-v1 per-cloud transforms and their orthogonality regulariser under autograd
 * (csrc/v1_transform.hip), forward and backward, every sum in a stated order.
 * Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19.
 * Reference: torch.bmm of the 3x3 input transform and the 64x64 feature transform with the
 * points, model/pointnet_utils.py:102-113, 120-123 and pose.py:50-69, and
 * feature_transform_reguliarzer, pointnet_utils.py:140-147, under the training loops' autograd.
 * Every entry is async on the caller's stream and graph-capturable, uses no float atomics, and
 * no workgroup waits for, or reads, another's result within a launch.  The unit is compiled
 * without contraction: an fma is only where a rule says "fma" (one rounding per step), every
 * other operation rounds on its own.  1 <= k <= 64 (the reference uses 3 and 64).
 *
 * Tensors of points -- x, y, dy, dx: [B][N][k] float32 -- are read and written in place through
 * ELEMENT strides (sb, sn, sc) >= 0: a channel-first [B][k][N] tensor is (k*N, 1, N), rows
 * [B][N][k] are (N*k, k, 1); any other view works too.  16-byte accesses are used only where a
 * tensor's base address, its strides and k allow them (unit sc with k, sn, sb multiples of 4, or
 * unit sn with sc, sb multiples of 4, and a 16-byte aligned base), dword accesses otherwise; no
 * access passes an edge.  T is [B][k][k] float32 with row stride ldt >= k (cloud b at
 * T + b*k*ldt).  dT, G are dense [B][k][k].
 *
 * pn2_transform_points_f32: y[b][n][i] = sum_j T[b][i][j] * x[b][n][j].
 *   THE RULE: each element is ONE float32 chain acc = fma(T[b][i][j], x[b][n][j], acc) over
 *   j = 0 .. k-1 from +0.0f.  ROW INDEPENDENCE: y[b][n][:] is a function of x[b][n][:] and of
 *   T[b] only -- not of N, B, the strides, the access width or the row's position.
 * pn2_transform_points_backward_f32: dy, and x (for dT), T (for dx) -> dx and dT; either output
 *   may be NULL and is then skipped (with what only it reads).  Every element of a non-NULL
 *   output is written: the buffers may hold anything.
 *   THE dx RULE: dx[b][n][j] = sum_i dy[b][n][i] * T[b][i][j], ONE float32 fma chain over
 *   i = 0 .. k-1 from +0.0f; row independent as the forward.
 *   THE dT RULE:
 *   1. the N rows of a cloud are cut into slabs of R = pn2_transform_slab_rows() rows, a
 *      constant of the build (a function of nothing): slab s holds rows [s*R, min((s+1)*R, N));
 *   2. slab s gives, per (i, j), the float64 partial P_s = sum_n double(dy[b][n][i]) *
 *      double(x[b][n][j]) over its rows in ascending n from +0.0 (each product is exact in
 *      float64; one rounding per add);
 *   3. dT[b][i][j] = float32(sum_s P_s) in ascending s from +0.0 in float64, rounded once.
 *   dT[b] therefore depends on cloud b's rows only -- not on B or on the other clouds.
 *   One launch writes the partials to `workspace` (8-byte aligned), a second one reduces them.
 *   pn2_transform_workspace_bytes(B, N, k) = B * ceil(N/R) * k * k * 8 bytes exactly (-1: bad
 *   arguments).  No workspace is needed (NULL, 0) when dT is NULL.
 *
 * pn2_orthogonality_forward_f32: T -> norm [B], loss (one float32), and G [B][k][k] when G is
 *   not NULL.
 *     G[b] = T[b] T[b]^T - I: G[b][i][j] is ONE float32 chain acc = fma(T[b][i][l], T[b][j][l],
 *       acc) over l = 0 .. k-1 from +0.0f, then one float32 subtraction of 1 where i == j.  The
 *       fma is symmetric in its two factors, so G[b] is BITWISE SYMMETRIC.
 *     norm[b] = float32(sqrt(sum double(G[b][i][j])^2)): ONE float64 chain over (i, j) in
 *       row-major order from +0.0 (each square exact), a correctly rounded float64 sqrt.
 *     loss = float32((sum_b double(norm[b])) / B), ascending b from +0.0.
 *   Two launches: the clouds side by side, then the mean.  norm is what the backward reads.
 * pn2_orthogonality_backward_f32: T, the forward's norm, dloss (a DEVICE pointer to the
 *   upstream float32 scalar) -> dT[b] = c_b * (G[b] T[b]):
 *     G[b] recomputed under the forward's rule;
 *     (G T)[i][j] ONE float32 chain acc = fma(G[b][i][l], T[b][l][j], acc) over l = 0 .. k-1
 *       from +0.0f, then one float32 multiplication by c_b;
 *     c_b = float32((2.0 * double(dloss)) / (double(B) * double(norm[b]))), rounded once.
 *   norm[b] == 0 (T[b] T[b]^T == I exactly): c_b = +0.0f, so dT[b] is all zeros -- what torch's
 *   CPU backward of torch.norm(..., dim=(1, 2)) gives at a zero matrix (it fills the norm's
 *   subgradient with zeros there instead of dividing by the norm).
 *
 * Errors, before any device call: PN2_EINVAL for B < 1, N < 1, k < 1, a negative stride, ldt
 * below k, a NULL required pointer (dx and dT both NULL included), a workspace that is too small
 * or not 8-byte aligned; PN2_EUNSUPPORTED for k > 64, B or N above 2^30, more than 2^31 - 1
 * 64-row tiles in all. */
int64_t pn2_transform_slab_rows(void);
int64_t pn2_transform_workspace_bytes(int64_t B, int64_t N, int64_t k);
int pn2_transform_points_f32(const float *x, int64_t xsb, int64_t xsn, int64_t xsc, const float *T,
                             int64_t ldt, float *y, int64_t ysb, int64_t ysn, int64_t ysc, int64_t B,
                             int64_t N, int64_t k, void *stream);
int pn2_transform_points_backward_f32(const float *dy, int64_t dsb, int64_t dsn, int64_t dsc,
                                      const float *x, int64_t xsb, int64_t xsn, int64_t xsc,
                                      const float *T, int64_t ldt, float *dx, int64_t gsb, int64_t gsn,
                                      int64_t gsc, float *dT, int64_t B, int64_t N, int64_t k,
                                      void *workspace, int64_t workspace_bytes, void *stream);
int pn2_orthogonality_forward_f32(const float *T, int64_t ldt, int64_t B, int64_t k, float *G, float *norm,
                                  float *loss, void *stream);
int pn2_orthogonality_backward_f32(const float *T, int64_t ldt, const float *norm, const float *dloss,
                                   int64_t B, int64_t k, float *dT, void *stream);

/* ---- the optimizer step of a train step as one launch over every tensor (csrc/optim.hip).
 * Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19.
 * Reference: every train script steps torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-08,
 * weight_decay=args.decay_rate), or SGD(lr=0.01, momentum=0.9) under --optimizer SGD, after each
 * batch, with StepLR(step_size=20, gamma=0.7) on top (train_classification.py:88-101, 128 and the
 * other train_*.py alike).  pn2/optim.py is the host side.
 *
 * THE TABLES.  `tensors` is a DEVICE array of ntensors descriptors; `tensors_host` is the
 * caller's HOST copy of the same array, read only by the argument check (the two must be equal:
 * the kernel trusts the device copy's pointers and counts as it trusts any pointer argument).
 * p, g, m, v are dense float32 arrays of n elements: the parameter, its gradient, and Adam's
 * exp_avg and exp_avg_sq (for SGD m is the momentum_buffer, or NULL for a tensor without one,
 * which then takes the plain update; v is not read).  `scalars` is the index of the tensor's
 * scalar block.  `jobs` is a DEVICE array of njobs int32 pairs (tensor, chunk): workgroup w
 * updates elements [chunk*C, min((chunk+1)*C, n)) of that tensor, C = pn2_optim_chunk() (2048, a
 * constant of the build).  Every (tensor, chunk) with chunk*C < n appears exactly once, so njobs
 * is the sum over the tensors of ceil(n / C); the order is free.  A pair that points outside the
 * tables or past n is skipped by the kernel, never followed.
 * 16-byte accesses are used for a whole chunk when the tensor's p, g, m and v base pointers are
 * all 16-byte aligned, dword accesses otherwise (a partial last chunk, an unaligned base); both
 * compute the same bits.  No LDS, no atomics, no cross-lane traffic: an element depends on its
 * own p, g, m, v and its scalar block only.
 *
 * THE SCALARS LIVE IN DEVICE MEMORY, never in kernel arguments: `scalars` holds nblocks blocks of
 * pn2_optim_scalars() (8) float32, which the host writes, stream-ordered, before each step.  A
 * launch captured into a hipGraph therefore replays with the values written for THAT replay
 * (the next step's bias corrections, a learning rate a scheduler changed).  The host computes
 * them in float64 with the expressions below and rounds each to float32 once.
 *   Adam block: [0] ss = -(lr / bc1), bc1 = 1 - beta1**step;  [1] bc2_sqrt = (1 - beta2**step)
 *               ** 0.5;  [2] omb1 = 1 - beta1;  [3] beta2;  [4] omb2 = 1 - beta2;  [5] eps;
 *               [6] wd = weight_decay;  [7] unused.
 *   SGD block:  [0] lr;  [1] mu = momentum;  [2] omd = 1 - dampening;  [3] wd = weight_decay;
 *               [4] first: nonzero on the step that creates the tensor's momentum_buffer;
 *               [5..7] unused.
 *
 * THE ARITHMETIC RULE.  Every operation is ONE correctly rounded IEEE float32 operation
 * (round to nearest even, subnormals kept), in this order, with no contraction:
 *   pn2_adam_step_f32, per element:
 *     g' = g + wd*p              only when wd != 0 (else g' = g)
 *     m  = m + omb1*(g' - m)
 *     v  = v*beta2;  v = v + (omb2*g')*g'
 *     den = sqrt(v) / bc2_sqrt + eps
 *     p  = p + ss*(m / den)
 *   pn2_sgd_step_f32, per element (torch's _single_tensor_sgd order):
 *     g' = g + wd*p              only when wd != 0
 *     with a buffer:  buf = g' when first != 0 (the buffer is written, not read), else
 *                     buf = buf*mu + omd*g';   then g' = buf
 *     p  = p - lr*g'
 *   Nesterov momentum, maximize and amsgrad are not built.  tests/optim_ref.py restates both
 *   rules with numpy float32 operators and gives the kernels' bits.
 *
 * Errors, before any device call: PN2_EINVAL for a NULL table or scalar pointer, a NULL p or g
 * (for Adam also m or v) in a descriptor, ntensors < 1 or nblocks < 1, a count n that is < 1 or
 * >= 2^31, a scalar index outside [0, nblocks), njobs that does not match the tensors' chunk
 * count; PN2_EUNSUPPORTED for more than 2^30 chunks. */
typedef struct pn2_optim_tensor {
    float *p;
    const float *g;
    float *m;
    float *v;
    int64_t n;
    int64_t scalars;
} pn2_optim_tensor;
int64_t pn2_optim_chunk(void);
int64_t pn2_optim_scalars(void);
int pn2_adam_step_f32(const pn2_optim_tensor *tensors_host, const pn2_optim_tensor *tensors,
                      int64_t ntensors, const int32_t *jobs, int64_t njobs, const float *scalars,
                      int64_t nblocks, void *stream);
int pn2_sgd_step_f32(const pn2_optim_tensor *tensors_host, const pn2_optim_tensor *tensors, int64_t ntensors,
                     const int32_t *jobs, int64_t njobs, const float *scalars, int64_t nblocks,
                     void *stream);

/* One shared-MLP layer packed for the kernels: wt = W^T pair-interleaved, [cin_pad/2][cout][2]
 * (element (k, o) at ((k>>1)*cout + o)*2 + (k&1), zero rows past cin), alpha[cout], beta[cout]
 * such that layer(x) = relu(alpha * (W x) + beta): the eval-mode BatchNorm2d folded with the
 * conv bias.  The kernels lay a row out as [features | xyz]; `rot` is the number of leading
 * input channels of W that are xyz (C for sample_and_group / group_all first layers, whose
 * reference order is [xyz, features]; 0 otherwise): row k of wt is input channel (k+rot)%cin.
 * cin_pad = pn2_layer_cin_pad(cin). */
int64_t pn2_layer_cin_pad(int64_t cin);
int pn2_pack_layer_f32(const float *W, const float *bias, const float *gamma, const float *beta,
                       const float *mean, const float *var, double eps, int64_t cout,
                       int64_t cin, int64_t rot, float *wt, float *alpha, float *beta_out,
                       void *stream);

/* Source of the MLP's input rows. */
#define PN2_SRC_GROUP_XYZ_FIRST 0  /* sample_and_group:  [xyz-ctr, feat] rows of group idx   */
#define PN2_SRC_GROUP_FEAT_FIRST 1 /* MSG:               [feat, xyz-ctr] rows of group idx   */
#define PN2_SRC_GROUP_ALL 2        /* sample_and_group_all: [xyz (raw), feat] of every point */
#define PN2_SRC_ROWS 3             /* a dense [M][cin] float32 matrix (row stride rs)        */

typedef struct pn2_mlp_layer {
    const float *wt;    /* [cin_pad][cout] */
    const float *alpha; /* [cout] */
    const float *beta;  /* [cout] */
    int64_t cin;
    int64_t cout;
    const void *wt_split; /* pn2_pack_layer_split_bf16 image of the same W, or NULL */
    int64_t flags;        /* PN2_LAYER_* bits, 0 = the SA layers' conv + BN + ReLU       */
} pn2_mlp_layer;

/* Layer without the ReLU: out = alpha * (W x) + beta (PointNetEncoder's conv3 + bn3 before its
 * max, /root/reference/model/pointnet_utils.py:125-127).  Served by the split dense-layer
 * kernels only (group_all / rows sources); other kernels reject it with PN2_EUNSUPPORTED.  The
 * training entry points (pn2_bn_relu_apply_f32 / pn2_bn_relu_backward_f32) take it as their
 * flags argument. */
#define PN2_LAYER_NO_RELU 1
/* pn2_bn_relu_backward_f32 only: mean / invstd are the caller's running statistics (eval-mode,
 * "frozen" BatchNorm), constants of the backward. */
#define PN2_LAYER_FROZEN_STATS 2

/* The same W packed for the split chain / dense kernels.  Planes 0-2: three bf16 planes (hi, mid,
 * lo with W = hi + mid + lo to 2^-24 relative), each [cout/32][kblocks][64 lanes][8] in MFMA
 * fragment order; planes 3-4: two fp16 planes (hi, lo) of W[o][.] * 2^e_o in the same order,
 * e_o putting output row o's largest |w| in [2^14, 2^15) (W*2^e = hi + lo to 2^-22 relative);
 * then float [cout] = 2^-e_o.  Kernel input channel k (block k/16) maps to W's input channel as
 * follows:
 *   xyz == 0 (hidden layers): k.   xyz > 0 (first layer, rows [xyz | features], D = cin-xyz):
 *   block 0 holds the xyz channels (k < xyz), blocks >= 1 the features (k-16 < D); W's own
 *   order is [xyz, features] if xyz_first (sample_and_group) else [features, xyz] (MSG).
 * Lane 32h + r, element j of fragment (t, kb) holds W[32t + r][in(16kb + (j&3) + 8(j>>2) + 4h)]
 * (0 for padding).  kblocks = pn2_layer_split_kblocks(cin, xyz); the image takes
 * pn2_layer_split_bytes(cout, cin, xyz) bytes, 16-byte aligned.  Chains given wt_split for
 * every layer (3 layers, grouped rows, hidden widths 32..128) run as one register-resident
 * kernel with fp32-accurate arithmetic: split fp16 (3 MFMAs per product, both operands scaled
 * by powers of two) where the chain's layer-0 input is register-resident or pre-transformed,
 * else split bf16 (6 MFMAs per product); others (and tuning mlp_f32 = 1) use the fp32 MFMA
 * kernels. */
int64_t pn2_layer_split_kblocks(int64_t cin, int64_t xyz);
int64_t pn2_layer_split_bytes(int64_t cout, int64_t cin, int64_t xyz);
int pn2_pack_layer_split_bf16(const float *W, int64_t cout, int64_t cin, int64_t xyz,
                              int xyz_first, void *out, void *stream);

/* Side job of an SA MLP call (pn2_sa_src.fps_side): the NEXT SA layer's farthest point sampling
 * -- pn2_fps_host_ws_f32's arguments, start_host[B] in host memory (read during the call).  It
 * runs inside the call's chain launch as extra workgroups when that launch allows it (its layer-0
 * input register-resident; B <= 256 clouds of N <= 512 points with C = 3 or 10, S <= 8192, its
 * LDS within the chain's), overlapping the MLP, else as its own launch on the same stream; the
 * same results either way.  Its inputs must not be written by the call; it needs no workspace
 * (pn2_fps_workspace_bytes == 0, else PN2_EINVAL).  In the reference the next layer samples
 * after this one's MLP (pointnet2_cls_ssg.py:27-28; the same draw order, the draws taken on the
 * host before the call). */
typedef struct pn2_fps_side {
    const float *pts; int64_t B, N, C, sb, sn, sc; /* points[b,n,c] = pts[b*sb + n*sn + c*sc]  */
    const int64_t *start_host;                      /* [B], host memory                       */
    int64_t S;
    int64_t *out_idx; float *out_pts; float *out_packed; float *pts_packed; /* as pn2_fps_f32 */
} pn2_fps_side;

typedef struct pn2_sa_src {
    int mode; /* PN2_SRC_* */
    const float *pts; int64_t pb, pn, pc; /* points [B,N,C], any strides            */
    const float *feat; int64_t fb, fn;    /* features [B,N,D], channel stride 1, or NULL */
    const float *ctr;                     /* centroids [B,S,C] contiguous (group modes) */
    const int64_t *idx;                   /* [B,S,K] int64 contiguous (group modes)     */
    const float *rows; int64_t rs;        /* PN2_SRC_ROWS: [M][rs]                      */
    int64_t B, N, C, D, S, K;             /* rows M = B*S*K (GROUP_ALL: S=1, K=N)       */
    const int32_t *cnt;                   /* [B,S] distinct neighbours per group
                                             (pn2_ball_query_cnt_f32), or NULL: group
                                             modes then compute only those rows          */
    float *zero_out; int64_t zero_count;  /* side job, or NULL: zero_count floats to zero
                                             (group_all's new_points, the reference's
                                             torch.zeros(B,1,C), pointnet2_utils.py:136),
                                             done by one of the call's launches          */
    const int32_t *idx32;                 /* [B,S,K] int32 (pn2_ball_query_i32), read in
                                             place of idx when not NULL (group modes)    */
    const pn2_fps_side *fps_side;         /* side job, or NULL (see pn2_fps_side)        */
} pn2_sa_src;

/* Bytes of workspace pn2_sa_mlp_max_f32 needs for this layer chain: 0 when the chain runs as
 * one fused kernel (every hidden width <= 256 and a compiled tile signature), otherwise two
 * [M][max hidden width] float32 buffers for the layer-by-layer path.  -1 on invalid input. */
int64_t pn2_sa_mlp_workspace_bytes(const pn2_sa_src *src, const pn2_mlp_layer *layers,
                                   int nlayers);

/* Fused gather -> nlayers x (1x1 conv + BN + ReLU) -> output.
 *   pool != 0 : out[g*ostride + c] = max over the K rows of group g (g = b*S+s) -- the
 *               torch.max(new_feature, 2)[0] of the reference, stored channels-last.
 *   pool == 0 : out[row*ostride + c] (dense rows, feeds a following PN2_SRC_ROWS call).
 * nlayers in [1,4]; every cout must be a multiple of 32.  Hidden activations stay in LDS; the
 * last layer is computed in 256-column slices (and split over the grid when nlayers == 1).
 * workspace may be NULL when pn2_sa_mlp_workspace_bytes() returns 0. */
int pn2_sa_mlp_max_f32(const pn2_sa_src *src, const pn2_mlp_layer *layers, int nlayers,
                       int pool, float *out, int64_t ostride, float *workspace,
                       int64_t workspace_bytes, void *stream);

/* The same fused SA MLP in bf16 arithmetic (BASELINE config 5, "features/MLP in bf16"):
 * every layer reads its input rounded to bf16 (round-to-nearest-even) and the hi plane of its
 * pn2_pack_layer_split_bf16 image (= bf16(W)); products are exact, accumulation, BN, ReLU and
 * the max are fp32, `out` is fp32.  Same arguments as pn2_sa_mlp_max_f32; every layer needs
 * wt_split.  Chains the register-resident chain kernel or the dense-layer kernel do not cover
 * return PN2_EUNSUPPORTED (no silent fp32 fallback).  Workspace: the _bf16 size query.
 * Replaces nothing in the reference (it has no bf16 path): same interface as
 * model/pointnet2_utils.py:167-172 at a lower precision, chosen by the caller. */
int64_t pn2_sa_mlp_workspace_bytes_bf16(const pn2_sa_src *src, const pn2_mlp_layer *layers,
                                        int nlayers);
int pn2_sa_mlp_max_bf16(const pn2_sa_src *src, const pn2_mlp_layer *layers, int nlayers,
                        int pool, float *out, int64_t ostride, float *workspace,
                        int64_t workspace_bytes, void *stream);

/* ---- input preparation (the step before the path) ----
 * pts: a DataLoader batch as float64 [B,N,C] (np.loadtxt rows), element (b,n,c) at
 * pts[b*sb + n*sn + c*sc].  For every cloud b, in float64 with numpy's operation order:
 *   mean_out[b*C + c] (or NULL) = float32(np.mean(points[b, :3, c]))  -- the first 3 POINTS, as
 *       test_translation.py:73 takes them, before normalising
 *   normalize != 0: xyz' = (xyz - centroid) / max_n |xyz_n - centroid|  (provider.normalization:
 *       centroid = sequential row sum / N, |v| = sqrt((x*x + y*y) + z*z)); C >= 3
 *   out[(b*N + n)*(C+K) + c] = float32(xyz'_c) (c < 3), float32(p[c]) (3 <= c < C),
 *       1.0f if c - C == labels[b] else 0.0f (C <= c < C+K, K = num_category; 0 = no splice)
 * out is the [B,N,C+K] float32 storage whose transpose(2,1) view is the model input (the
 * layout the reference's scripts hand the model).  labels: int64 [B] device, each in [0, K)
 * (checked by the caller: the reference raises IndexError).  1 <= C <= 64. */
int pn2_prepare_points_f64(const double *pts, int64_t B, int64_t N, int64_t C, int64_t sb,
                           int64_t sn, int64_t sc, int normalize, const int64_t *labels,
                           int64_t num_category, float *out, float *mean_out, void *stream);
/* The training scripts' preparation (train_translation.py:109-119; train_rotation.py:108-116
 * without the mean): pn2_prepare_points_f64 on the batch the augmentations leave, with the
 * draws made by the caller (pn2.provider.draw_augmentation consumes numpy's generator as the
 * reference does).  The value of point n, channel c that everything above consumes is
 *   p = pts[b, drop[b*N + n] ? 0 : n, c]            random_point_dropout (provider.py:157-164):
 *                                                   a dropped row is row 0's, all C channels
 *   c < 3:  p = fl(fl(p * scale[b]) + shift[b*3 + c])   random_scale_point_cloud, then
 *                                                   shift_point_cloud: two roundings, no FMA
 *   c >= 3: p unchanged
 * so mean_out is the mean of the first min(3,N) AUGMENTED points, and the centroid, the max
 * norm and the divide see the augmented cloud.  drop: uint8 [B,N] (non-zero = dropped), scale:
 * float64 [B], shift: float64 [B,3]; device pointers, each NULL to skip that stage (all three
 * NULL computes exactly pn2_prepare_points_f64).  pts is not written. */
int pn2_prepare_train_points_f64(const double *pts, int64_t B, int64_t N, int64_t C, int64_t sb,
                                 int64_t sn, int64_t sc, int normalize, const int64_t *labels,
                                 int64_t num_category, const uint8_t *drop, const double *scale,
                                 const double *shift, float *out, float *mean_out, void *stream);

/* ---- training (batch-statistics BatchNorm) around library GEMMs; rows are channels-last
 * [M][C] with row stride ld.  Workspace: pn2_bn_train_workspace_bytes(M, C) bytes (float64
 * chunk partials), caller-owned. ----
 * Column statistics of Y: mean, invstd = 1/sqrt(var_biased + eps); sxhat[c] = sum_r xhat
 * (float64, for the conv bias gradient); when momentum > 0 also
 * running_mean/var = (1-momentum)*old + momentum*(mean, var_unbiased) (torch's rule). */
int64_t pn2_bn_train_workspace_bytes(int64_t M, int64_t C);
int pn2_bn_train_stats_f32(const float *Y, int64_t M, int64_t C, int64_t ld, double eps,
                           double momentum, float *running_mean, float *running_var, float *mean,
                           float *invstd, double *sxhat, void *ws, int64_t ws_bytes, void *stream);
/* A = relu((Y - mean) * invstd * gamma + beta); flags PN2_LAYER_NO_RELU: no ReLU. */
int pn2_bn_relu_apply_f32(const float *Y, int64_t M, int64_t C, int64_t ld, const float *mean,
                          const float *invstd, const float *gamma, const float *beta, float *A,
                          int64_t lda, int flags, void *stream);
/* pn2_bn_train_stats_f32 then pn2_bn_relu_apply_f32 in one call (one host crossing per layer):
 * stats = [mean | invstd], 2*C floats. */
int pn2_bn_train_forward_f32(const float *Y, int64_t M, int64_t C, int64_t ld, double eps,
                             double momentum, float *running_mean, float *running_var,
                             const float *gamma, const float *beta, float *A, int64_t lda, int flags,
                             float *stats, double *sxhat, void *ws, int64_t ws_bytes, void *stream);
/* out[g*ldo + c] = max over k < K of A[(g*K + k)*lda + c]; arg[g*C + c] = first argmax (int32);
 * NaN is the maximum (first NaN), as torch.max. */
int pn2_group_max_f32(const float *A, int64_t G, int64_t K, int64_t C, int64_t lda, float *out,
                      int64_t ldo, int32_t *arg, void *stream);
/* Backward of A = relu(bn_train(Y)): dXn = dA * [A > 0] (dA with flags PN2_LAYER_NO_RELU, the
 * backward of A = bn_train(Y)), with dA dense (ldd) or, when dA is
 * NULL, scattered from the max: dA[r][c] = dOut[r/K][c] if arg[r/K][c] == r%K else 0.
 * dbeta = sum_r dXn, dgamma = sum_r dXn*xhat (float64 sums, of float64 products), and
 * dY = gamma*invstd*(dXn - dbeta/M - xhat*dgamma/M); dbias (or NULL) = sum_r dY, the preceding
 * conv's bias gradient, from the forward's sxhat. */
int pn2_bn_relu_backward_f32(const float *Y, int64_t M, int64_t C, int64_t ld, const float *mean,
                             const float *invstd, const float *gamma, const float *beta,
                             const float *dA, int64_t ldd, const float *dOut, int64_t ldo,
                             const int32_t *arg, int64_t K, const double *sxhat, float *dY,
                             int64_t ldy, float *dgamma, float *dbeta, float *dbias, void *ws,
                             int64_t ws_bytes, int flags, void *stream);
/* With flags PN2_LAYER_FROZEN_STATS the same entry is the backward of A = relu(bn_eval(Y)):
 * mean / invstd are running statistics, dXn, dbeta and dgamma as above,
 * dY = gamma*invstd*dXn (no batch-statistics correction), dbias = gamma*invstd*dbeta; sxhat is
 * not read and may be NULL. */
/* pn2_bn_relu_apply_f32 followed by pn2_group_max_f32 in one pass over Y, without writing A:
 * out[g*ldo + c] = max over k < K of act((Y[(g*K + k)*ld + c] - mean)*invstd*gamma + beta),
 * arg[g*C + c] = its first argmax (int32), NaN the maximum; out and arg are bit-identical to the
 * two calls.  flags: PN2_LAYER_NO_RELU. */
int pn2_bn_relu_group_max_f32(const float *Y, int64_t G, int64_t K, int64_t C, int64_t ld,
                              const float *mean, const float *invstd, const float *gamma,
                              const float *beta, float *out, int64_t ldo, int32_t *arg, int flags,
                              void *stream);

/* ---- small-batch fully connected layer (the eval FC tails, BN folded into W / bias on the
 * host): out[b*ldo + n] = act(sum_k x[b*ldx + k] * W[n*K + k] + bias[n]) for b < B (rows in
 * blocks of 16; each element computed the same way whatever B is),
 * W row-major [N][K], bias may be NULL; flags PN2_LINEAR_RELU applies the ReLU.  Float32 FMA.
 * Reference: pointnet_utils.py:33-40, pointnet_cls.py:26-28, rotation.py:45-49. ---- */
#define PN2_LINEAR_RELU 1
int pn2_linear_rows_f32(const float *x, int64_t ldx, int64_t B, int64_t K, const float *W,
                        const float *bias, float *out, int64_t ldo, int64_t N, int flags,
                        void *stream);

/* ---- the PointNet++ heads' eval FC tail in three launches: fc1 + bn1 + ReLU, fc2 + bn2 + ReLU
 * (as pn2_linear_rows_f32), then fc3 fused with the classifiers' log_softmax over the N3 logits
 * and the first argmax of each row (PN2_TAIL_LOGSOFTMAX) -- pointnet2_cls_ssg.py:31-38
 * (F.log_softmax(x, -1), x.data.max(1)[1]), the same tails of pointnet2_cls_msg.py,
 * rotation_ssg.py, translation_ssg.py, sign_ssg.py.  BN is folded into W / bias on the host;
 * dropout is the identity in eval.  x [B][K] (row stride ldx), W1 [N1][K], W2 [N2][N1],
 * W3 [N3][N2] row-major; out [B][N3] (row stride ldo): the log-probabilities with the flag, else
 * the fc3 outputs; argmax [B] int64 or NULL.  fc1 and fc2 elements are computed as
 * pn2_linear_rows_f32 computes them; each fc3 element is the in-order sum of four float32 fma
 * chains over consecutive quarters of k (the same whatever B is).  N3 <= 819.  workspace:
 * pn2_fc_tail_workspace_bytes(B, N1, N2) bytes, 16-byte aligned (y1 and y2). */
#define PN2_TAIL_LOGSOFTMAX 1
int64_t pn2_fc_tail_workspace_bytes(int64_t B, int64_t N1, int64_t N2);
int pn2_fc_tail_f32(const float *x, int64_t ldx, int64_t B, int64_t K, const float *W1,
                    const float *b1, int64_t N1, const float *W2, const float *b2, int64_t N2,
                    const float *W3, const float *b3, int64_t N3, int flags, float *out,
                    int64_t ldo, int64_t *argmax, void *workspace, int64_t workspace_bytes,
                    void *stream);

/* Which kernel family served this thread's last successful pn2_sa_mlp_max_* call:
 * PN2_PATH_F32 (fp32 MFMA kernels), PN2_PATH_SPLIT_BF16 (split-bf16 chain / dense kernels) or
 * PN2_PATH_BF16 (pn2_sa_mlp_max_bf16). */
#define PN2_PATH_F32 1
#define PN2_PATH_SPLIT_BF16 2
#define PN2_PATH_BF16 3
int pn2_sa_mlp_last_path(void);
/* Planes per operand of the MLP kernels of this thread's last successful pn2_sa_mlp_max_* call:
 * 3 (split bf16: 6 MFMAs per product), 2 (split fp16: 3), 1 (bf16), 0 (fp32 MFMA kernels). */
int pn2_sa_mlp_last_planes(void);
/* Where this thread's last pn2_sa_mlp_max_* call ran its FPS side job (pn2_sa_src.fps_side):
 * 1 inside the chain launch (extra workgroups of that launch), 0 as its own launch after the
 * MLP, -1 the call had no side job (ABI 17). */
int pn2_sa_mlp_last_fps_side(void);

/* ---- runtime: CU-partitioned streams (pipelined serving, pn2/pipeline.py) ---- */
int pn2_device_cu_count(int device, int *count);
/* A stream whose kernels run only on the CUs set in mask (bit i of word i/32 = CU i). */
int pn2_stream_create_cu_masked(int device, const uint32_t *mask, int mask_words, void **stream);
int pn2_stream_destroy(void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PN2_H */
