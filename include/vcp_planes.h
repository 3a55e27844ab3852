/*
 * vcp_planes.h -- plane extraction by consensus (RANSAC) on the device: the entry points of csrc/planes.hip.  They live in
 * libvcp.so beside those of vcp.h, whose conventions (contexts, status codes, host and _dev forms, the vcp_set_stream
 * contract, no CPU fallback) hold here unchanged.  DESIGN.md section 36.
 *
 * Most returns of a scan that are not targets lie on a few large planes (the floor, the walls behind the targets).  Left in
 * the cloud they become giant DBSCAN clusters that vcp_cluster_shapes refuses and the moments filter throws away afterwards.
 * vcp_plane_ransac finds the dominant planes by consensus and labels their rows, so that the rest can be clustered.
 *
 * Definition, shared by every function below.  All arithmetic binary64, every operation rounded on its own (no FMA
 * contraction), / and sqrt correctly rounded.  Row i is pts[i * ld + 0 .. 3), ld >= 3 in doubles: columns of a wider
 * resident array are read in place.
 *   residual of row i against the plane (a, b, c, d):   r = fl(fl(fl(fl(a x) + fl(b y)) + fl(c z)) + d)
 *   inlier:                                             fabs(r) <= thr        (false for NaN)
 *   active row:                                         active == NULL or active[i] != 0
 *   plane of the triple (i0, i1, i2), with p_j = row i_j:
 *       u = p1 - p0, v = p2 - p0 (componentwise)
 *       cx = fl(fl(uy vz) - fl(uz vy)),  cy = fl(fl(uz vx) - fl(ux vz)),  cz = fl(fl(ux vy) - fl(uy vx))
 *       nrm = sqrt(fl(fl(fl(cx cx) + fl(cy cy)) + fl(cz cz)))
 *       (a, b, c) = (cx / nrm, cy / nrm, cz / nrm);   d = -fl(fl(fl(a p0x) + fl(b p0y)) + fl(c p0z))
 *     valid when every index is in [0, n), nrm is finite and > 0, and a, b, c, d are finite; otherwise valid = 0 and the
 *     plane is four NaN (0x7FF8000000000000), which no row is an inlier of.  There is no sign convention.
 *   score:  count[h] = the number of active rows that are inliers of plane h (integers: independent of any order).
 */
#ifndef VCP_PLANES_H
#define VCP_PLANES_H
#include "vcp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The shape of the score kernel on the context's device: shape[0] = the rows one workgroup takes per trip (tile),
 * shape[1] = the hypotheses one pass over the cloud scores (chunk), shape[2] = the largest grid (workgroups) it launches.
 * A call with more than shape[2] tiles makes workgroups take several tiles; one with H > shape[1] makes several passes.
 * VCP_ERR_ARG: NULL ctx or shape.  Launches nothing. */
int vcp_plane_score_shape(vcp_ctx* ctx, int32_t shape[3]);

/* counts[h] = the score (above) of plane h = planes[h * 4 + 0 .. 4) over the active rows, h = 0 .. H - 1.
 *   pts, ld, n     the rows (above); n == 0: every count is 0
 *   active         [n] uint8 or NULL
 *   planes         [H * 4] doubles (a, b, c, d); a plane holding a NaN scores 0
 *   thr            the inlier bound; 0 and +inf are allowed
 *   counts         [H] int64
 * Errors, found before any output is touched; nothing is written on an error.  VCP_ERR_ARG: NULL ctx, planes or counts,
 * NULL pts with n > 0, n < 0, ld < 3, H < 1 or H > 65536, !(thr >= 0) (NaN and negative bounds); VCP_ERR_TOO_LARGE:
 * n >= 0x7FFFFFF0, as vcp_centroids_dev.  The result is a function of the input alone: two calls give identical counts,
 * and so does a call after any other call on the context.  Timing phase: planes_score (csrc/planes.hip). */
int vcp_plane_score(vcp_ctx* ctx, const double* pts, int64_t ld, int64_t n, const uint8_t* active, const double* planes,
                    int32_t H, double thr, int64_t* counts);
/* Same with device pointers for pts, active, planes and counts, on the context's stream under the vcp_set_stream contract;
 * returns when the counts are in place. */
int vcp_plane_score_dev(vcp_ctx* ctx, const double* d_pts, int64_t ld, int64_t n, const uint8_t* d_active,
                        const double* d_planes, int32_t H, double thr, int64_t* d_counts);

/* planes[h * 4 + 0 .. 4) = the plane (above) of the triple tri[h * 3 + 0 .. 3), valid[h] (may be NULL) = its validity.
 * Device pointers: d_tri [H * 3] int32, d_planes [H * 4] doubles, d_valid [H] uint8; on the context's stream under the
 * vcp_set_stream contract; returns when the result is in place.  An index outside [0, n) makes the plane invalid, it is
 * not an error and no row is read through it.
 * Errors, found before any output is touched; nothing is written on an error.  VCP_ERR_ARG: NULL ctx, d_tri or d_planes,
 * NULL d_pts with n > 0, n < 0, ld < 3, H < 1 or H > 65536; VCP_ERR_TOO_LARGE: n >= 0x7FFFFFF0.  Timing phase:
 * planes_sample. */
int vcp_planes_from_triples_dev(vcp_ctx* ctx, const double* d_pts, int64_t ld, int64_t n, const int32_t* d_tri, int32_t H,
                                double* d_planes, uint8_t* d_valid);

/* Every active row that is an inlier of `plane` (four doubles in host memory) gets labels[i] = id and, where d_active is
 * not NULL, active[i] = 0; every other row of labels and active is untouched.  *n_labelled = the rows labelled.
 * Device pointers: d_active [n] uint8 in/out or NULL, d_labels [n] int32 in/out; on the context's stream under the
 * vcp_set_stream contract; returns when the result is in place.
 * Errors, found before any output is touched; nothing is written on an error.  VCP_ERR_ARG: NULL ctx, plane or n_labelled,
 * NULL d_pts or d_labels with n > 0, n < 0, ld < 3, !(thr >= 0); VCP_ERR_TOO_LARGE: n >= 0x7FFFFFF0.  Timing phase:
 * planes_label. */
int vcp_plane_label_dev(vcp_ctx* ctx, const double* d_pts, int64_t ld, int64_t n, uint8_t* d_active, const double plane[4],
                        double thr, int32_t id, int32_t* d_labels, int64_t* n_labelled);

/* Plane extraction.  Sampling: mix(seed, c) is splitmix64 of the counter c, every step modulo 2^64:
 *       z = seed + 0x9E3779B97F4A7C15 (c + 1);  z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) 0x94D049BB133111EB;
 *       mix = z ^ z >> 31
 *   (mix(0, 0) = 0xE220A8397B1DCDAF, mix(0, 1) = 0x6E789E6AA1B965F4, mix(0, 2) = 0x06C45D188009454F,
 *   mix(1234567, 0) = 0x599ED017FB08FC85).  act = the m active rows in ascending index.  In round r hypothesis h takes
 *   member j = 0, 1, 2 as act[(mix(seed, (r H + h) 3 + j) m) >> 64], the high half of the 128-bit product.  A repeated
 *   member gives nrm = 0: the hypothesis is invalid.
 * Rounds r = 0, 1, ... while r < max_planes:
 *   1. stop if m < 3;
 *   2. the H planes of the round's triples (above), scored over the active rows;
 *   3. the winner is the largest count, on a tie the lowest h; stop if that count is < max(min_inliers, 3);
 *   4. with refit != 0: vcp_cluster_moments (vcp.h) with dim 3, K = 1, no weights and the label 1 for the winner's active
 *      inliers, 0 for every other row, by its own definition.  The refit plane has (a, b, c) = row 2 of evec (the axis of
 *      the smallest eigenvalue) and d = -fl(fl(fl(a m0) + fl(b m1)) + fl(c m2)) with m its mean.  It is taken when the
 *      moments' valid is 1 and its count over the active rows is >= the winner's; otherwise the winner is kept;
 *   5. the active inliers of the accepted plane take the label r + 1 and leave the active set;
 *   6. planes[r * 4 + 0 .. 4) = the accepted plane, counts[r] = the rows labelled, hyp_counts[r] = the winner's count.
 * Outputs: labels [n] int32 (0 = on no plane; written for every row, inactive ones included), *n_planes = the planes
 * accepted; planes [max_planes * 4], counts and hyp_counts [max_planes] in host memory, the entries from *n_planes on
 * NaN (0x7FF8000000000000) and 0.  active is read only.
 *   n == 0:            VCP_OK, *n_planes = 0;    max_planes == 0:  VCP_OK, *n_planes = 0, every label 0
 * Errors, found before any output is touched; nothing is written on an error.  VCP_ERR_ARG: NULL ctx or n_planes, NULL pts
 * or labels with n > 0, NULL planes, counts or hyp_counts with max_planes > 0, n < 0, ld < 3, H < 1 or H > 65536,
 * max_planes < 0 or > 64, min_inliers < 0, !(thr >= 0); VCP_ERR_TOO_LARGE: n >= 0x7FFFFFF0.
 * The loop runs in the library; per round a few words come back to the host (m, the winner, the refit's count, the rows
 * labelled).  The result is a function of the input alone: two calls give identical bits, and so does a call after any
 * other call on the context.  Timing phases, once per round: planes_sample (the active list, the triples, their planes),
 * planes_score (the H counts and the winner), planes_refit, planes_label (csrc/planes.hip). */
int vcp_plane_ransac(vcp_ctx* ctx, const double* pts, int64_t ld, int64_t n, const uint8_t* active, double thr, int32_t H,
                     int32_t max_planes, int64_t min_inliers, uint64_t seed, int32_t refit, int32_t* labels, double* planes,
                     int64_t* counts, int64_t* hyp_counts, int32_t* n_planes);
/* Same with device pointers for pts, active and labels, on the context's stream under the vcp_set_stream contract; planes,
 * counts, hyp_counts and n_planes stay in host memory. */
int vcp_plane_ransac_dev(vcp_ctx* ctx, const double* d_pts, int64_t ld, int64_t n, const uint8_t* d_active, double thr,
                         int32_t H, int32_t max_planes, int64_t min_inliers, uint64_t seed, int32_t refit, int32_t* d_labels,
                         double* planes, int64_t* counts, int64_t* hyp_counts, int32_t* n_planes);

#ifdef __cplusplus
}
#endif
#endif /* VCP_PLANES_H */
