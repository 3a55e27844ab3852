// ICP.cs -- drop-in replacement for vtkPointCloud/BaseClass/ICP.cs: go_hell_ICP keeps its signature and
// writes R (3x3 Matrix) and T (3x1 Matrix) in place (caller: FrmMain.cs:2685-2690).  The arithmetic is the
// intended Besl-McKay/Horn loop; the shipped body cannot run past round 1 (see SURVEY.md fact 4).
using System;
using System.Collections.Generic;

namespace vtkPointCloud
{
    class ICP
    {
        public int maxIter = 1000;

        static double[] Flatten(List<Point3D> l)
        {
            double[] a = new double[3 * l.Count];
            for (int i = 0; i < l.Count; i++) { a[3 * i] = l[i].X; a[3 * i + 1] = l[i].Y; a[3 * i + 2] = l[i].Z; }
            return a;
        }

        public void go_hell_ICP(List<Point3D> model, List<Point3D> data, Matrix R, Matrix T, double e)
        {
            if (data.Count == 0) return;
            double[] r = new double[9], t = new double[3];
            double sse, rmse; int iters;
            using (VcpNative.Lease c = VcpNative.Rent())
                VcpNative.Check(c, VcpNative.vcp_icp(c.Ctx, Flatten(model), model.Count, Flatten(data), data.Count, e,
                maxIter, VcpNative.VCP_STOP_SSE_DELTA, r, t, out sse, out rmse, out iters));
            if (iters == 1 && sse < e) return;
            for (int i = 0; i < 3; i++)
            {
                for (int j = 0; j < 3; j++) R[i, j] = r[3 * i + j];
                T[i, 0] = t[i];
            }
        }

        // Global registration by congruent pairs (vcp.h: vcp_register_pairs; new, no counterpart in the reference): a pose
        // of `source` on `target` without any start.  bases = pairs of source indices (2 per base); every base is laid on
        // every ordered pair of targets of its own planar length within lenTol, and each such pose is scored by the source
        // landmarks it puts within inlierDist of some target.  Returns the best base (-1: no base has a matching target
        // pair, M16 is then the identity); M16 receives its row-major 4x4 matrix, inliers / score (may be null) the
        // per-base counts.
        public int RegisterPairs(List<Point3D> source, List<Point3D> target, int[] bases, double lenTol, bool mirror,
            double inlierDist, double[] M16, int[] inliers, int[] score)
        {
            int best;
            using (VcpNative.Lease c = VcpNative.Rent())
                VcpNative.Check(c, VcpNative.vcp_register_pairs(c.Ctx, Flatten(source), source.Count, Flatten(target),
                target.Count, bases, bases.Length / 2, lenTol, mirror ? 1 : 0, 200, inlierDist, M16, out best, null, score,
                inliers, null, null));
            return best;
        }

        // RegisterPairs where `source` is not in the targets' unit (vcp.h: vcp_register_sim): a base fits an ordered pair
        // of targets whose length is k times its own, scaleMin <= k <= scaleMax, and the pose in M16 is the planar
        // similarity with that k.  scale (may be null) receives the winner's k per base, 0 where a base found nothing.
        public int RegisterSimilarity(List<Point3D> source, List<Point3D> target, int[] bases, double scaleMin,
            double scaleMax, bool mirror, double inlierDist, double[] M16, int[] inliers, int[] score, double[] scale)
        {
            int best;
            using (VcpNative.Lease c = VcpNative.Rent())
                VcpNative.Check(c, VcpNative.vcp_register_sim(c.Ctx, Flatten(source), source.Count, Flatten(target),
                target.Count, bases, bases.Length / 2, scaleMin, scaleMax, mirror ? 1 : 0, 200, inlierDist, M16, out best,
                null, score, inliers, null, null, scale));
            return best;
        }
    }
}
