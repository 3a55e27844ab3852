/*
 * vcp_features.h -- the local surface at every return: normal, eigenvalues and surface variation of the neighbourhood
 * covariance, and the mean distance to the neighbours; the entry points of csrc/point_features.hip.  They live in
 * libvcp.so beside those of vcp.h, whose conventions (contexts, status codes, host and _dev forms, the vcp_set_stream
 * contract, no CPU fallback) hold here unchanged.  DESIGN.md section 37.
 *
 * The neighbour rows are the caller's: usually the knn of vcp_kdist, whose order is pinned (ascending (distance, index)).
 * Because the order of a row's neighbours is pinned, every sum below is pinned, and tests/point_features_ref.py restates
 * the whole call in numpy for equality.
 *
 * Definition.  All arithmetic binary64, every operation rounded on its own (no FMA contraction), / and sqrt correctly
 * rounded.  Row i is pts[i * ld + 0 .. dim), dim 2 or 3, ld >= dim in doubles: columns of a wider resident array are read
 * in place.  nbr is [n * k] int32, 1 <= k <= 64.  Slot s of row i is a MEMBER when 0 <= nbr[i * k + s] < n; any other
 * value (the -1 of vcp_kdist, anything out of range) is skipped: it is not an error and no row is read through it.  The
 * members are taken in slot order j_0 .. j_(m-1); a repeated index counts as often as it appears; whether i is in its own
 * row is the caller's business (vcp_kdist puts it there unless k or more lower-indexed duplicates exist).  SUM means
 * acc = +0.0; acc = fl(acc + term) in slot order.  x_a(j) is coordinate a of row j, p_i the row i itself.
 *   1. count[i] = m
 *   2. mean_a = (SUM x_a(j_t)) / (double)m
 *   3. d_a(t) = fl(x_a(j_t) - mean_a);  S_ab = SUM fl(d_a(t) d_b(t)) for a <= b;  cov_ab = S_ab / (double)m
 *      (centred, in two passes, for the reason vcp_cluster_moments gives: a cloud far from the origin keeps its digits)
 *   4. eval[i * dim ..) and evec = sym_eig<dim> (csrc/symeig.hpp) of cov: descending eigenvalues, its sign and NaN rules
 *   5. normal[i * dim ..) = row dim - 1 of evec, the axis of the smallest eigenvalue.  With viewpoint != NULL:
 *      v_a = fl(viewpoint_a - p_i,a), s = the left-to-right sum of fl(n_a v_a); the normal is negated (exact) when s < 0
 *      and stays as it is when s == 0 or s is NaN.  The test uses the row p_i, not the mean.
 *   6. variation[i] = eval[dim - 1] / sum, sum = the left-to-right sum of eval; +0 when sum == 0, NaN when eval is NaN
 *   7. mean_dist[i] = (SUM dist_t) / (double)q over the members with j_t != i, in slot order, q their number;
 *      dist_t = sqrt(left-to-right sum of fl(e_a e_a)), e_a = fl(x_a(j_t) - p_i,a);  q == 0 gives NaN
 *   8. valid[i] = 1 when m >= dim and every entry of mean and cov is finite, else 0.
 *      m == 0: every double output is NaN, valid 0.  0 < m < dim: every output is what steps 2 - 7 give, valid 0 (a single
 *      finite member: cov +0, evec the identity, so the normal is the last unit vector).
 * Every NaN written is 0x7FF8000000000000.
 */
#ifndef VCP_FEATURES_H
#define VCP_FEATURES_H
#include "vcp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The shape of the kernel on the context's device: shape[0] = the rows one workgroup takes per trip, shape[1] = the
 * largest grid (workgroups) it launches, shape[2 .. 6) = the k classes it is instantiated for, ascending (a call runs the
 * smallest class >= k; classes up to shape[3] keep the gathered rows in registers between the two passes, the larger ones
 * gather again).  A call with more than shape[0] * shape[1] rows makes workgroups take several trips.
 * VCP_ERR_ARG: NULL ctx or shape.  Launches nothing. */
int vcp_point_features_shape(vcp_ctx* ctx, int32_t shape[6]);

/* The features (above) of every row.
 *   pts, ld, dim, n   the rows
 *   nbr, k            the neighbour rows [n * k] int32
 *   viewpoint         dim doubles in HOST memory (both forms), or NULL: the sign is left to sym_eig's rule
 *   normal, eval      [n * dim] doubles;   variation, mean_dist  [n] doubles;   count [n] int32;   valid [n] uint8
 * Every output pointer may be NULL; with all of them NULL the call returns VCP_OK and launches nothing.  Outputs must not
 * overlap inputs.  n == 0: VCP_OK.
 * Errors, found before any output is touched; nothing is written on an error.  VCP_ERR_ARG: NULL ctx, n < 0, dim not 2 or
 * 3, ld < dim, k < 1, NULL pts or nbr with n > 0; VCP_ERR_UNSUPPORTED: k > 64; VCP_ERR_TOO_LARGE: n >= 0x7FFFFFF0.
 * The result is a function of the input alone (no atomics, no workspace read that the call did not write): two calls give
 * identical bits, and so does a call after any other call on the context.  Timing phase: features_rows. */
int vcp_point_features(vcp_ctx* ctx, const double* pts, int64_t ld, int dim, int64_t n, const int32_t* nbr, int k,
                       const double* viewpoint, double* normal, double* eval, double* variation, double* mean_dist,
                       int32_t* count, uint8_t* valid);
/* Same with device pointers for everything but viewpoint, on the context's stream under the vcp_set_stream contract;
 * returns when the outputs are in place.  Needs no workspace. */
int vcp_point_features_dev(vcp_ctx* ctx, const double* d_pts, int64_t ld, int dim, int64_t n, const int32_t* d_nbr, int k,
                           const double* viewpoint, double* d_normal, double* d_eval, double* d_variation,
                           double* d_mean_dist, int32_t* d_count, uint8_t* d_valid);

#ifdef __cplusplus
}
#endif
#endif /* VCP_FEATURES_H */
