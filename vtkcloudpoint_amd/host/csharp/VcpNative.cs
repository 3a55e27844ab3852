// VcpNative.cs -- P/Invoke declarations for libvcp.so / vcp.dll (include/vcp.h).  Drop next to the classes
// in vtkPointCloud/BaseClass/.  NOT COMPILED IN THIS REPO'S IMAGE (no dotnet/mono/csc here): kept as the
// reference-side binding a maintainer adds; the executable mirrors are ../cpp/vcp_host.hpp and the Python
// package.  Target: .NET Framework 3.5+ (blittable arrays are pinned by the marshaller, no copies).
// The library is 64-bit only (ROCm) and exports cdecl: build the host AnyCPU/x64, not the reference project's default
// x86 (vtkPointCloud.csproj:61,71) -- every DllImport names the convention, and Ctx refuses a 32-bit process.
using System;
using System.Runtime.InteropServices;

namespace vtkPointCloud
{
    internal static class VcpNative
    {
        const string Lib = "vcp";   // libvcp.so on Linux (Mono/.NET), vcp.dll on Windows

        public const int VCP_L1_2D = 0, VCP_L2_2D = 1, VCP_L2_3D = 2, VCP_SIGNED_SUM_2D = 3;
        public const int VCP_STOP_SSE_DELTA = 0, VCP_STOP_RMSE = 1;

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_create(int device_id, out IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void vcp_destroy(IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern IntPtr vcp_last_error(IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_release_workspace(IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_selftest_scan_dev(IntPtr ctx, IntPtr d_in, IntPtr d_out, long n, int op, out uint total);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_dbscan(IntPtr ctx, double[] coords, long n, int dim, int metric,
            double eps, int min_pts, int cf_in, byte[] in_mask, byte[] in_classed, int[] labels, byte[] is_core,
            byte[] is_classed, out int cf_out, out long dist_evals);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_dbscan_blocks(IntPtr ctx, double[] motor, long n, double eps,
            int min_pts, int pts_in_cell, int small_max, int[] labels, int[] block_of, long[] merge_order, out long m_out,
            out int rows, out int cols, out int kept, out int del_sum, out int cluster_amount, out long dist_evals);

        // MainForm.getClusterFromList (FrmMain.cs:1136-1213): partition on (X, Y), DBImproved on motor
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_dbscan_blocks_keyed(IntPtr ctx, double[] key_xy,
            double[] motor, long n, double eps, int min_pts, int pts_in_cell, int small_max, int[] labels, int[] block_of,
            long[] merge_order, out long m_out, out int rows, out int cols, out int kept, out int del_sum,
            out int cluster_amount, out long dist_evals);

        // Tools.getFixedPtsCentroid (Tools.cs:78-111)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_centroids_weighted(IntPtr ctx, double[] xyz,
            int[] group, int[] cluster_id, int[] pts_count, long n, int K, int ignore_duplication, double[] c3,
            long[] inside_num);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_centroids(IntPtr ctx, double[] xyz, double[] motor, int[] labels,
            long n, int K, double[] c3, double[] c2, long[] counts);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_merge_centroids(IntPtr ctx, double[] cxy, int[] ids, int K,
            double thr, int[] map_to, out int merge_count);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp(IntPtr ctx, double[] model, long nm, double[] data, long nd,
            double tol, int max_iter, int stop_rule, double[] R, double[] T, out double sse, out double rmse, out int iters);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_match(IntPtr ctx, double[] centers, int K, double[] truths, int T,
            double[] M, double max_dist, double[] matched_xyz, byte[] is_matched, int[] nearest, double[] nearest_dist,
            out int count_matched);
        // the one-to-one pairing (no truth twice); matched_xyz and pair_dist may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_match_unique(IntPtr ctx, double[] centers, int K, double[] truths,
            int T, double[] M, double max_dist, double[] matched_xyz, int[] truth_of, int[] center_of, double[] pair_dist,
            out int count_pairs, out int rounds);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_match_unique_dev(IntPtr ctx, IntPtr d_centers, int K, IntPtr d_truths,
            int T, double[] M, double max_dist, IntPtr d_matched_xyz, IntPtr d_truth_of, IntPtr d_center_of,
            IntPtr d_pair_dist, out int count_pairs, out int rounds);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_refresh_by_dictionary(IntPtr ctx, double[] xyz, double[] motor,
            int[] labels, long n, int K, int[] map_by_id, out int new_k, double[] c3, double[] c2, long[] counts);

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp_sums(IntPtr ctx, double[] model, long nm, double[] data, long nd,
            double[] R, double[] T, double[] sums, int[] nn);

        // MainForm.ICP() (FrmMain.cs:841-907): the knobs it sets on vtkIterativeClosestPointTransform
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp_vtklike(IntPtr ctx, double[] source, long ns, double[] target,
            long nt, int max_iter, int max_landmarks, int start_by_matching_centroids, double[] M, out double mean_dist,
            out int iters);

        // the same loop from n_poses start rotations (null init_R: Rz(h * 2 pi / n_poses)), best pose by inliers;
        // M_all, mean_dist and inliers may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp_multistart(IntPtr ctx, double[] source, long ns, double[] target,
            long nt, int n_poses, double[] init_R, double[] init_T, int max_iter, int max_landmarks, double inlier_dist,
            double[] M_best, out int best, double[] M_all, double[] mean_dist, int[] inliers);

        // gated ICP (vcp.h): a pair whose distance is >= the round's gate stays out of the sums.  One pass (the test
        // handle; nn and keep may be null) and vcp_icp_multistart with a schedule: round r uses gates[min(r, n_gates) - 1];
        // kept and starved may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp_sums_gated(IntPtr ctx, double[] model, long nm, double[] data,
            long nd, double[] R, double[] T, double gate, double[] sums, out long kept, int[] nn, byte[] keep);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp_gated(IntPtr ctx, double[] source, long ns, double[] target,
            long nt, int n_poses, double[] init_R, double[] init_T, int max_iter, int max_landmarks, double[] gates,
            int n_gates, int min_pairs, double inlier_dist, double[] M_best, out int best, double[] M_all,
            double[] mean_dist, int[] inliers, long[] kept, int[] starved);

        // trimmed ICP (vcp.h): every round fits on the m pairs with the smallest distances.  One round's passes (the test
        // handle; nn and keep may be null) and vcp_icp_multistart with a schedule of keep shares: round r keeps
        // ceil(keep[min(r, n_keep) - 1] * landmarks) pairs; kept, starved and trim_dist may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp_sums_trimmed(IntPtr ctx, double[] model, long nm, double[] data,
            long nd, double[] R, double[] T, long m, double[] sums, out double thr_dd, int[] nn, byte[] keep);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp_trimmed(IntPtr ctx, double[] source, long ns, double[] target,
            long nt, int n_poses, double[] init_R, double[] init_T, int max_iter, int max_landmarks, double[] keep,
            int n_keep, int min_pairs, double inlier_dist, double[] M_best, out int best, double[] M_all,
            double[] mean_dist, int[] inliers, long[] kept, int[] starved, double[] trim_dist);

        // unique-correspondence ICP (vcp.h): of the landmarks that share a nearest target only the closest may enter a
        // round's sums; the gate then decides on it.  One round's passes (the test handle; nn and keep may be null; keep:
        // 1 kept, 0 winner dropped by the gate, 2 not the winner) and vcp_icp_gated with that rule; kept, starved and lost
        // may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp_sums_unique(IntPtr ctx, double[] model, long nm, double[] data,
            long nd, double[] R, double[] T, double gate, double[] sums, out long kept, int[] nn, byte[] keep, out long lost);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp_unique(IntPtr ctx, double[] source, long ns, double[] target,
            long nt, int n_poses, double[] init_R, double[] init_T, int max_iter, int max_landmarks, double[] gates,
            int n_gates, int min_pairs, double inlier_dist, double[] M_best, out int best, double[] M_all,
            double[] mean_dist, int[] inliers, long[] kept, int[] starved, long[] lost);

        // similarity ICP (vcp.h): the gated loop whose rounds also fit one isotropic scale, the product of the factors held
        // in [ratio_min, ratio_max] (ratio_min <= 1 <= ratio_max).  One pass (the test handle: vcp_icp_sums_gated with
        // sums [18]; nn and keep may be null), the step on the host (returns 1, 2 = scale not determined, 0 = failed; V may
        // be null with use_v = 0) and the loop; kept, starved, ratio and unscaled may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp_sums_sim(IntPtr ctx, double[] model, long nm, double[] data,
            long nd, double[] R, double[] T, double gate, double[] sums, out long kept, int[] nn, byte[] keep);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_selftest_horn_sim(double[] sums, long n, double[] V, int use_v, double c,
            double ratio_min, double ratio_max, double[] R1s, double[] T1, out double k_used, out double c_new);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp_sim(IntPtr ctx, double[] source, long ns, double[] target,
            long nt, int n_poses, double[] init_R, double[] init_T, int max_iter, int max_landmarks, double[] gates,
            int n_gates, int min_pairs, double ratio_min, double ratio_max, double inlier_dist, double[] M_best,
            out int best, double[] M_all, double[] mean_dist, int[] inliers, long[] kept, int[] starved, double[] ratio,
            int[] unscaled);

        // anisotropic ICP: vcp_icp_gated whose round fits one scale for x and one for y, pose y = R diag(sx, sy, 1) d + t.
        // One pass (the test handle: sums [18] over the raw landmarks under the pose A, T; nn and keep may be null), the
        // step on the host (returns 1, 0 = failed; determined: bit a = axis a; V may be null with use_v = 0) and the loop;
        // init_scale [2 n_poses] may be null (all 1), as may kept, starved, scale [2 n_poses] and unscaled [2 n_poses]
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp_sums_aniso(IntPtr ctx, double[] model, long nm, double[] data,
            long nd, double[] A, double[] T, double gate, double[] sums, out long kept, int[] nn, byte[] keep);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_selftest_horn_aniso(double[] sums, long n, double[] V, int use_v, double[] R,
            double[] s, double[] lo, double[] hi, double[] R_new, double[] T_new, double[] s_new, out int determined);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp_aniso(IntPtr ctx, double[] source, long ns, double[] target,
            long nt, int n_poses, double[] init_R, double[] init_T, double[] init_scale, int max_iter, int max_landmarks,
            double[] gates, int n_gates, int min_pairs, double ratio_min, double ratio_max, double inlier_dist,
            double[] M_best, out int best, double[] M_all, double[] mean_dist, int[] inliers, long[] kept, int[] starved,
            double[] scale, int[] unscaled);

        // congruent-pair global registration (no counterpart in the reference; bases = pairs of source indices)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_register_pairs(IntPtr ctx, double[] source, long ns, double[] target,
            long nt, int[] bases, int n_bases, double len_tol, int mirror, int max_landmarks, double inlier_dist,
            double[] M_best, out int best, double[] M_all, int[] score, int[] inliers, int[] pick, long[] n_hyp);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_register_pairs_dev(IntPtr ctx, IntPtr d_source, long ns, IntPtr d_target,
            long nt, IntPtr d_bases, int n_bases, double len_tol, int mirror, int max_landmarks, double inlier_dist,
            double[] M_best, out int best, IntPtr d_M_all, IntPtr d_score, IntPtr d_inliers, IntPtr d_pick, IntPtr d_n_hyp);

        // scale-free registration by similarity pairs (vcp.h): vcp_register_pairs where a base fits a target pair whose
        // length is k times its own, scale_min <= k <= scale_max; scale receives the winner's k per base (may be null)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_register_sim(IntPtr ctx, double[] source, long ns, double[] target,
            long nt, int[] bases, int n_bases, double scale_min, double scale_max, int mirror, int max_landmarks,
            double inlier_dist, double[] M_best, out int best, double[] M_all, int[] score, int[] inliers, int[] pick,
            long[] n_hyp, double[] scale);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_register_sim_dev(IntPtr ctx, IntPtr d_source, long ns, IntPtr d_target,
            long nt, IntPtr d_bases, int n_bases, double scale_min, double scale_max, int mirror, int max_landmarks,
            double inlier_dist, double[] M_best, out int best, IntPtr d_M_all, IntPtr d_score, IntPtr d_inliers, IntPtr d_pick,
            IntPtr d_n_hyp, IntPtr d_scale);

        // Tools.getCircles / Geometry.FindMinimalBoundingCircle (Tools.cs:394-409, Geometry.cs:247-319)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_mcc(IntPtr ctx, double[] xy, int[] labels, long[] order, long m, long n,
            int K, double[] centers, double[] radius, byte[] valid, int[] hull_n);

        // hull + circle + minimum-area bounding rectangle of every cluster (vcp.h, "cluster shapes"); every array after
        // valid may be null (hull_off / hull_idx: both or neither)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_cluster_shapes(IntPtr ctx, double[] xy, int[] labels, long[] order, long m,
            long n, int K, double[] centers, double[] radius, byte[] valid, int[] hull_n, double[] rect_xy, double[] rect_len,
            int[] rect_edge, byte[] rect_valid, int[] hull_off, int[] hull_idx);

        // MainForm.FilterClustersByRadius (FrmMain.cs:1905-1920) with the length / width criterion beside it, and the
        // stable removal of Tools.removeFilterPointFromClustering (Tools.cs:70-74); rect_len / rect_valid, keep, kept_idx may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_cluster_filter(IntPtr ctx, int[] labels, long n, int K, double[] radius,
            byte[] valid, double[] rect_len, byte[] rect_valid, double max_radius, double max_aspect, byte[] filtered,
            byte[] keep, int[] kept_idx, out int n_filtered, out long n_kept);

        // per-row work of MainForm.AddFolder (FrmMain.cs:1011-1090)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_import_convert(IntPtr ctx, double[] rows, long n, double x_angle,
            double y_angle, int xdir, int ydir, int dedupe, double[] xyz, byte[] state, out long kept, out long duplicates);

        // the same with the kept rows written densely and the size of every duplicate class; group = the file number is
        // AddFolder's typpe 3 / 4 (FrmMain.cs:1069-1085: count is Point3D.ptsCount).  Every array may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_import_compact(IntPtr ctx, double[] rows, long n, int[] group,
            double x_angle, double y_angle, int xdir, int ydir, int dedupe, double[] motor, double[] xyz, double[] dist,
            int[] src, int[] count, int[] group_out, int[] row_to, out long m, out long duplicates);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_import_compact_dev(IntPtr ctx, IntPtr d_rows, long n, IntPtr d_group,
            double x_angle, double y_angle, int xdir, int ydir, int dedupe, IntPtr d_motor, IntPtr d_xyz, IntPtr d_dist,
            IntPtr d_src, IntPtr d_count, IntPtr d_group_out, IntPtr d_row_to, out long m, out long duplicates);

        // the scan files' text parsed on the GPU (vcp.h: vcp_parse_scan_text; what FileMap.ReadFile + Convert.ToDouble do,
        // FrmMain.cs:1005-1009): text = File.ReadAllBytes of the files one after the other, each ending with '\n';
        // seg_off [nseg + 1] their offsets (null: one file).  rows == null / d_rows == IntPtr.Zero counts the lines;
        // VCP_ERR_UNSUPPORTED (-8) means bytes outside the device reader's set: read that file the old way.  err [3]
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_parse_scan_text(IntPtr ctx, byte[] text, ulong nbytes, ulong[] seg_off,
            int nseg, long cap, double[] rows, int[] group, long[] seg_first, out long n, out long n_host, long[] err);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_parse_scan_text_dev(IntPtr ctx, byte[] text, ulong nbytes, ulong[] seg_off,
            int nseg, long cap, IntPtr d_rows, IntPtr d_group, long[] seg_first, out long n, out long n_host, long[] err);

        // the exports' text built on the GPU (vcp.h: vcp_format_rows; what the WriteLine loops of Tools.cs:233, 295, 341, 374
        // write): line j = [id[r] TAB] a[r * stride_a] TAB b[..] TAB c[..] EOL, r = order[j] (null: r = j, m == n), "F<bit>";
        // eol 1 = "\r\n" (StreamWriter.WriteLine).  text == null counts the bytes into nbytes; VCP_ERR_UNSUPPORTED (-8)
        // means a NaN, an infinity or 1e15 and more: write that file the old way.  err [2]
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_format_rows(IntPtr ctx, int[] id, double[] a, long stride_a,
            double[] b, long stride_b, double[] c, long stride_c, long[] order, long n, long m, int bit, int eol,
            byte[] text, ulong cap, out ulong nbytes, long[] err);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_format_rows_dev(IntPtr ctx, IntPtr d_id, IntPtr d_a, long stride_a,
            IntPtr d_b, long stride_b, IntPtr d_c, long stride_c, IntPtr d_order, long n, long m, int bit, int eol,
            byte[] text, ulong cap, out ulong nbytes, long[] err);

        // order statistics per cluster or group (vcp.h: vcp_cluster_quantiles; per list what Tools.GetGroupingManOrMin,
        // Tools.cs:468-497, takes over all lists): values[i * stride], group 0 = none; counts may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_cluster_quantiles(IntPtr ctx, double[] values, long stride,
            int[] group, long n, int K, double[] q, int nq, double[] output, long[] counts);
        // mean, covariance, principal axes and the ellipse numbers of every cluster (vcp.h: vcp_cluster_moments): row i is
        // pts[i * ld + 0 .. dim), dim 2 or 3; weights may be null (1); every output may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_cluster_moments(IntPtr ctx, double[] pts, long ld, int dim,
            int[] labels, int[] weights, long n, int K, double[] mean, double[] cov, double[] eval, double[] evec, double[] shape,
            byte[] valid, long[] counts);
        // least-squares sphere (dim 3) or circle (dim 2) of every cluster (vcp.h: vcp_cluster_spheres): pts, ld, dim, labels and
        // weights as in vcp_cluster_moments; fixed_radius 0 fits the radius, > 0 fixes it; rounds 0..64; every output may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_cluster_spheres(IntPtr ctx, double[] pts, long ld, int dim,
            int[] labels, int[] weights, long n, int K, double fixed_radius, int rounds, double[] centre, double[] radius, double[] rms,
            double[] cap, double[] step, double[] alg, byte[] valid, long[] counts);
        // a band of Distance per group from the median absolute deviation, where Tools.FilterByDistance_FixedPoint
        // (Tools.cs:438-461) applies one band to every file: reject[i] != 0 is Point3D.isFilterByDistance
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_cluster_mad(IntPtr ctx, double[] values, long stride,
            int[] group, long n, int K, double c_mad, double floor, double[] med, double[] mad, double[] thr, byte[] reject,
            long[] kept, out long n_rejected);

        // query of MainForm.refreshClusList (FrmMain.cs:3452-3456)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_assign_truths(IntPtr ctx, double[] motor, long n, double[] truths_xy,
            int[] truth_ids, int T, double radius, int[] ids, out long outliers);

        // k-distance graph for choosing eps (no reference counterpart: the dialogs take eps typed by hand,
        // Clustering.Designer.cs:86,96); knn may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_kdist(IntPtr ctx, double[] coords, long n, int dim, int metric,
            int k, double[] kdist, int[] knn);
        // eps tree: what DBImproved(minPts = k) decides at every eps <= eps_max (vcp.h: vcp_eps_tree; no reference
        // counterpart).  kdist: read when kdist_given != 0, else written (may be null); reach, merge_a / merge_b (both or
        // neither) may be null; merge_w, merge_a, merge_b have room for max(n - 1, 0) entries
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_eps_tree(IntPtr ctx, double[] coords, long n, int dim, int metric,
            int k, double eps_max, int kdist_given, double[] kdist, double[] reach, out long n_merge, double[] merge_w,
            int[] merge_a, int[] merge_b, out int rounds);

        // DBSCAN with point weights and a range gate (vcp.h: vcp_gdbscan; no reference counterpart).  aux (with gate),
        // weights, is_core and wsum may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_gdbscan(IntPtr ctx, double[] coords, long n, int dim, int metric,
            double eps, double[] aux, double gate, int[] weights, long min_weight, int cf_in, int[] labels, byte[] is_core,
            long[] wsum, out int cf_out);

        // ---- device-resident forms (IntPtr = device address): for hosts that keep the cloud on the GPU between
        // calls, and for the multi-GPU drivers (one process and one context per GPU) ----
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_dev_alloc(IntPtr ctx, ulong bytes, out IntPtr dptr);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_dev_free(IntPtr ctx, IntPtr dptr);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_h2d(IntPtr ctx, IntPtr dst_dev, double[] src_host, ulong bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_d2h(IntPtr ctx, int[] dst_host, IntPtr src_dev, ulong bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_dbscan_dev(IntPtr ctx, IntPtr d_coords, long n, int dim, int metric,
            double eps, int min_pts, int cf_in, IntPtr d_in_classed, IntPtr d_labels, IntPtr d_is_core, IntPtr d_is_classed,
            out int cf_out, out long dist_evals);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_centroids_dev(IntPtr ctx, IntPtr d_xyz, IntPtr d_motor, IntPtr d_labels,
            long n, int K, IntPtr d_c3, IntPtr d_c2, IntPtr d_counts);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_cluster_shapes_dev(IntPtr ctx, IntPtr d_xy, IntPtr d_labels, IntPtr d_order,
            long m, long n, int K, IntPtr d_centers, IntPtr d_radius, IntPtr d_valid, IntPtr d_hull_n, IntPtr d_rect_xy,
            IntPtr d_rect_len, IntPtr d_rect_edge, IntPtr d_rect_valid, IntPtr d_hull_off, IntPtr d_hull_idx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_cluster_filter_dev(IntPtr ctx, IntPtr d_labels, long n, int K,
            IntPtr d_radius, IntPtr d_valid, IntPtr d_rect_len, IntPtr d_rect_valid, double max_radius, double max_aspect,
            IntPtr d_filtered, IntPtr d_keep, IntPtr d_kept_idx, out int n_filtered, out long n_kept);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_kdist_dev(IntPtr ctx, IntPtr d_coords, long n, int dim, int metric,
            int k, IntPtr d_kdist, IntPtr d_knn);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_eps_tree_dev(IntPtr ctx, IntPtr d_coords, long n, int dim, int metric,
            int k, double eps_max, int kdist_given, IntPtr d_kdist, IntPtr d_reach, out long n_merge, IntPtr d_merge_w,
            IntPtr d_merge_a, IntPtr d_merge_b, out int rounds);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_gdbscan_dev(IntPtr ctx, IntPtr d_coords, long n, int dim, int metric,
            double eps, IntPtr d_aux, double gate, IntPtr d_weights, long min_weight, int cf_in, IntPtr d_labels, IntPtr d_is_core,
            IntPtr d_wsum, out int cf_out);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_cluster_quantiles_dev(IntPtr ctx, IntPtr d_values, long stride,
            IntPtr d_group, long n, int K, double[] q, int nq, IntPtr d_out, IntPtr d_counts);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_cluster_moments_dev(IntPtr ctx, IntPtr d_pts, long ld, int dim,
            IntPtr d_labels, IntPtr d_weights, long n, int K, IntPtr d_mean, IntPtr d_cov, IntPtr d_eval, IntPtr d_evec, IntPtr d_shape,
            IntPtr d_valid, IntPtr d_counts);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_cluster_spheres_dev(IntPtr ctx, IntPtr d_pts, long ld, int dim,
            IntPtr d_labels, IntPtr d_weights, long n, int K, double fixed_radius, int rounds, IntPtr d_centre, IntPtr d_radius, IntPtr d_rms,
            IntPtr d_cap, IntPtr d_step, IntPtr d_alg, IntPtr d_valid, IntPtr d_counts);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_cluster_mad_dev(IntPtr ctx, IntPtr d_values, long stride,
            IntPtr d_group, long n, int K, double c_mad, double floor, IntPtr d_med, IntPtr d_mad, IntPtr d_thr,
            IntPtr d_reject, IntPtr d_kept, out long n_rejected);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_icp_dev(IntPtr ctx, IntPtr d_model, long nm, IntPtr d_data, long nd,
            double tol, int max_iter, int stop_rule, double[] R, double[] T, out double sse, out double rmse, out int iters);
        // block pipeline in stages (per-block step sharded over GPUs, distributed.py: sharded_blocks)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_begin(IntPtr ctx, double[] motor, long n, double eps, int min_pts,
            int pts_in_cell, int small_max, out int rows, out int cols, out long nblocks, out long m);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_begin_dev(IntPtr ctx, IntPtr d_motor, long n, double eps,
            int min_pts, int pts_in_cell, int small_max, out int rows, out int cols, out long nblocks, out long m);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_begin_keyed(IntPtr ctx, double[] key_xy,
            double[] motor, long n, double eps, int min_pts, int pts_in_cell, int small_max, out int rows, out int cols,
            out long nblocks, out long m);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_begin_keyed_dev(IntPtr ctx, IntPtr d_key_xy,
            IntPtr d_motor, long n, double eps, int min_pts, int pts_in_cell, int small_max, out int rows, out int cols,
            out long nblocks, out long m);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_share(IntPtr ctx, int rank, int world, out int block_lo,
            out int block_hi, out long pos_lo, out long pos_hi);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_cluster_dev(IntPtr ctx, int block_lo, int block_hi, IntPtr d_local,
            out long evals);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_finish_dev(IntPtr ctx, IntPtr d_local, long evals_blocks,
            IntPtr d_labels, IntPtr d_block_of, IntPtr d_merge_order, out long m_out, out int kept, out int del_sum,
            out int cluster_amount, out long dist_evals);
        // one DBImproved.dbscan spread over several GPUs (distributed.py: exact_slabs)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_slab_begin(IntPtr ctx, IntPtr d_coords, long n, int dim, int metric,
            double eps, int min_pts, IntPtr d_noexpand, IntPtr d_ord, IntPtr d_rep, IntPtr d_is_core, out long n_comp);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_slab_comps(IntPtr ctx, uint[] comp_rep);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_slab_finish(IntPtr ctx, uint[] map_rep, uint[] map_k, long n_tab,
            int[] tab_gid, uint[] tab_seed, uint own_lo, uint own_count, IntPtr d_labels, IntPtr d_is_classed, out long twice);

        // ---- several GPUs from this one process (csrc/multi.hip): what the ThreadPool fan-out of FrmMain.cs:1356-1359
        // becomes -- one context and one native host thread per listed device, label slices gathered on device 0 ----
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_create_multi(int[] device_ids, int n, out IntPtr multi);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void vcp_destroy_multi(IntPtr multi);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern IntPtr vcp_multi_last_error(IntPtr multi);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_multi_count(IntPtr multi);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern IntPtr vcp_multi_ctx(IntPtr multi, int i);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_dbscan_blocks_multi(IntPtr multi, double[] key_xy,
            double[] motor, long n, double eps, int min_pts, int pts_in_cell, int small_max, int[] labels, int[] block_of,
            long[] merge_order, out long m_out, out int rows, out int cols, out int kept, out int del_sum,
            out int cluster_amount, out long dist_evals);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_share_plan(uint[] blockstart, long nblocks, int world, long[] cuts);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_selftest_horn(double[] sums, long nd, double[] V, int use_v, double[] R1, double[] T1);
        // the block pipeline with every stage sharded (include/vcp.h): one context per GPU, each building, clustering and
        // merging its own share of the blocks; the exchanges between the stages are the host's (ten words per rank, the
        // active noise points gathered for the one global noise pass, the (index, label) pairs) --
        // vtkcloudpoint_amd/distributed.py is the reference driver
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_plan_dev(IntPtr ctx, IntPtr d_key_xy, IntPtr d_motor, long n, double eps, int min_pts, int pts_in_cell, int small_max, out int rows, out int cols, out long nblocks, out long nsuper);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_plan_cuts(IntPtr ctx, int world, long[] cuts);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_build_dev(IntPtr ctx, long super_lo, long super_hi, out int block_lo, out int block_hi, out long m_loc, out long n_loc);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_finish_local_dev(IntPtr ctx, IntPtr d_local, long[] info8);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_finish_zero_dev(IntPtr ctx, int zero_last, out long z_count, out long active_count);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_finish_zcoords_dev(IntPtr ctx, int swap_xy, IntPtr d_zcoords);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_blocks_finish_pairs_dev(IntPtr ctx, int kept_offset, IntPtr d_zlab, IntPtr d_pairs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int vcp_scatter_pairs_dev(IntPtr ctx, IntPtr d_pairs, long count, long n, IntPtr d_labels);

        // The device set of the multi-GPU calls: created on first use from Devices (default: device 0 only), replaced when
        // Devices changes, destroyed by Shutdown().  One vcp_multi serves one call at a time (the lock below).
        public static int[] Devices = new int[] { 0 };
        static IntPtr multi = IntPtr.Zero;
        static int[] multiDevices = null;
        public static readonly object MultiLock = new object();
        public static IntPtr Multi   // call under lock (MultiLock)
        {
            get
            {
                bool same = multi != IntPtr.Zero && multiDevices != null && multiDevices.Length == Devices.Length;
                if (same) for (int i = 0; i < Devices.Length; i++) same &= multiDevices[i] == Devices[i];
                if (!same)
                {
                    if (multi != IntPtr.Zero) { vcp_destroy_multi(multi); multi = IntPtr.Zero; }
                    if (IntPtr.Size != 8) throw new InvalidOperationException("libvcp is 64-bit only");
                    int rc = vcp_create_multi(Devices, Devices.Length, out multi);
                    if (rc != 0) throw new InvalidOperationException("vcp_create_multi: " + Marshal.PtrToStringAnsi(vcp_multi_last_error(IntPtr.Zero)));
                    multiDevices = (int[])Devices.Clone();
                }
                return multi;
            }
        }
        public static void CheckMulti(int rc)
        {
            if (rc != 0) throw new InvalidOperationException("vcp error " + rc + ": " + Marshal.PtrToStringAnsi(vcp_multi_last_error(multi)));
        }

        // ---- contexts ---------------------------------------------------------------------------------------------
        // A context (stream + device workspace, ~100 bytes per point of its largest call) serves one call at a time.
        // StartCode runs on ThreadPool threads (FrmMain.cs:1358), which come and go: a context per thread would leak one
        // context and its workspace per retired thread.  Callers therefore RENT a context for the duration of a call --
        //     using (VcpNative.Lease c = VcpNative.Rent()) VcpNative.Check(c, VcpNative.vcp_dbscan(c.Ctx, ...));
        // -- and Dispose returns it to a per-device pool; at most MaxPooled idle contexts are kept per device, the rest
        // are destroyed on return.  Device selects the HIP ordinal new leases use (default 0); Shutdown() destroys
        // every idle context (call it from Application.ApplicationExit).
        public static int Device = 0;
        public static int MaxPooled = 4;
        static readonly object poolLock = new object();
        static readonly System.Collections.Generic.Dictionary<int, System.Collections.Generic.Stack<IntPtr>> pool =
            new System.Collections.Generic.Dictionary<int, System.Collections.Generic.Stack<IntPtr>>();

        public sealed class Lease : IDisposable
        {
            public IntPtr Ctx;
            public readonly int DeviceId;
            internal Lease(IntPtr c, int dev) { Ctx = c; DeviceId = dev; }
            public void Dispose()
            {
                IntPtr c = Ctx;
                Ctx = IntPtr.Zero;
                if (c == IntPtr.Zero) return;
                lock (poolLock)
                {
                    System.Collections.Generic.Stack<IntPtr> st;
                    if (!pool.TryGetValue(DeviceId, out st)) { st = new System.Collections.Generic.Stack<IntPtr>(); pool[DeviceId] = st; }
                    if (st.Count < MaxPooled) { st.Push(c); return; }
                }
                vcp_destroy(c);   // the pool is full: this context and its workspace go
            }
        }

        public static Lease Rent() { return Rent(Device); }
        public static Lease Rent(int device)
        {
            if (IntPtr.Size != 8) throw new InvalidOperationException("libvcp is 64-bit only: build the host x64 / AnyCPU without Prefer32Bit");
            lock (poolLock)
            {
                System.Collections.Generic.Stack<IntPtr> st;
                if (pool.TryGetValue(device, out st) && st.Count > 0) return new Lease(st.Pop(), device);
            }
            IntPtr c;
            int rc = vcp_create(device, out c);
            if (rc != 0) throw new InvalidOperationException("vcp_create(" + device + "): " + Marshal.PtrToStringAnsi(vcp_last_error(IntPtr.Zero)));
            return new Lease(c, device);
        }

        public static void Shutdown()
        {
            lock (poolLock)
            {
                foreach (System.Collections.Generic.Stack<IntPtr> st in pool.Values)
                    while (st.Count > 0) vcp_destroy(st.Pop());
                pool.Clear();
            }
            lock (MultiLock)
            {
                if (multi != IntPtr.Zero) vcp_destroy_multi(multi);
                multi = IntPtr.Zero;
                multiDevices = null;
            }
        }

        public static void Check(Lease c, int rc)
        {
            if (rc != 0) throw new InvalidOperationException("vcp error " + rc + ": " + Marshal.PtrToStringAnsi(vcp_last_error(c.Ctx)));
        }
    }
}
