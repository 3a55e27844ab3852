// MainForm.Gpu.cs -- the MainForm members on the hot path, as a drop-in: MainForm is already `partial`
// (FrmMain.cs / FrmMain.Designer.cs); delete calMatchedCoords + RecorrectMatchingPtsByDistance (FrmMain.cs:3572-3618),
// refreshClusList (:3437-3467), ICP() (:841-907), FilterClustersByRadius (:1905-1920) and removePointByRadius (:3743-3746)
// from FrmMain.cs, replace the row loop of AddFolder (:991-1090) by
// the call shown at AddScanRows below, and add this file.  Field names are the reference's own (centers, trues,
// rawData, clusList, circles, filterID, clusterSum, truePointCloud, truePointVertices, M, ren, vtkControl, matchedID, x_angle, y_angle, pathList,
// PtsInRegionTxt, toolStripStatusLabelCurrentPointCount, trueScale, centroidScale, scale, clock, clock_y, clock_x).
using System;
using System.Collections.Generic;
using System.Linq;
using System.Windows.Forms;

namespace vtkPointCloud
{
    public partial class MainForm
    {
        double[] gpuMatched;      // matched_X/Y/Z of every centroid, filled by calMatchedCoords
        int[] gpuNearest;
        double[] gpuNearestDist;

        static double[] Matrix16(vtk.vtkMatrix4x4 m)
        {
            double[] a = new double[16];
            for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) a[4 * r + c] = m.GetElement(r, c);
            return a;
        }

        double[] TruthArray()
        {
            int T = (int)truePointCloud.GetNumberOfPoints();
            double[] t = new double[3 * T];
            for (int i = 0; i < T; i++) { double[] p = truePointCloud.GetPoint(i); t[3 * i] = p[0]; t[3 * i + 1] = p[1]; t[3 * i + 2] = p[2]; }
            return t;
        }

        // FrmMain.cs:3572-3587.  The transform and the nearest-truth search are one native call; the distances are
        // kept for RecorrectMatchingPtsByDistance, which the UI calls again whenever the threshold changes.
        public void calMatchedCoords()
        {
            int K = centers.Count;
            if (K == 0) return;
            double[] c = new double[3 * K];
            for (int j = 0; j < K; j++) { c[3 * j] = centers[j].tmp_X; c[3 * j + 1] = centers[j].tmp_Y; c[3 * j + 2] = centers[j].tmp_Z; }
            gpuMatched = new double[3 * K];
            gpuNearest = new int[K];
            gpuNearestDist = new double[K];
            byte[] isM = new byte[K];
            int cnt;
            using (VcpNative.Lease lease = VcpNative.Rent())
                VcpNative.Check(lease, VcpNative.vcp_match(lease.Ctx, c, K, TruthArray(), (int)truePointCloud.GetNumberOfPoints(),
                Matrix16(M), double.PositiveInfinity, gpuMatched, isM, gpuNearest, gpuNearestDist, out cnt));
            for (int j = 0; j < K; j++)
            {
                centers[j].matched_X = gpuMatched[3 * j];
                centers[j].matched_Y = gpuMatched[3 * j + 1];
                centers[j].matched_Z = gpuMatched[3 * j + 2];
                centers[j].isMatched = false;
            }
        }

        // FrmMain.cs:3588-3618
        public void RecorrectMatchingPtsByDistance(double matchDistance, bool isShowUnmatchedCenterPts, bool isShowUnmatchedTruePts)
        {
            int countMatched = 0;
            matchedID = new List<int>();
            if (gpuNearest == null || gpuNearest.Length != centers.Count) calMatchedCoords();
            for (int j = 0; j < centers.Count; j++)
            {
                centers[j].isMatched = false;
                if (gpuNearestDist[j] < matchDistance)
                {
                    centers[j].isMatched = true;
                    centers[j].matchNum = gpuNearest[j];
                    matchedID.Add(gpuNearest[j]);
                    countMatched++;
                }
            }
            this.toolStripStatusLabelCurrentPointCount.Text = "总共" + centers.Count + "个聚类质心，总共" + truePointCloud.GetNumberOfPoints() + "个真值点，匹配" + countMatched + "个点";
            showMatchedLine(isShowUnmatchedCenterPts, isShowUnmatchedTruePts);
        }

        // RecorrectMatchingPtsByDistance as a pairing: the loop above lets a false cluster beside a target take the same
        // matchNum as the real one, so matchedID and the exported pair list (:1696-1698) hold that truth twice.  Here a
        // truth goes to one centroid only (vcp_match_unique: nearest pairs first, ties to the lower centroid, then the
        // lower truth index), so matchedID has no duplicates and unmatchedTruths is the complement the
        // isShowUnmatchedTruePts display wants.  Call it in place of RecorrectMatchingPtsByDistance; nothing else changes.
        public List<int> unmatchedTruths = new List<int>();

        public void MatchOneToOne(double matchDistance, bool isShowUnmatchedCenterPts, bool isShowUnmatchedTruePts)
        {
            int K = centers.Count, T = (int)truePointCloud.GetNumberOfPoints();
            matchedID = new List<int>();
            unmatchedTruths = new List<int>();
            int countMatched = 0, rounds = 0;
            if (K > 0)
            {
                double[] c = new double[3 * K];
                for (int j = 0; j < K; j++) { c[3 * j] = centers[j].tmp_X; c[3 * j + 1] = centers[j].tmp_Y; c[3 * j + 2] = centers[j].tmp_Z; }
                gpuMatched = new double[3 * K];
                int[] truthOf = new int[K], centerOf = new int[Math.Max(T, 1)];
                using (VcpNative.Lease lease = VcpNative.Rent())
                    VcpNative.Check(lease, VcpNative.vcp_match_unique(lease.Ctx, c, K, TruthArray(), T, Matrix16(M), matchDistance,
                        gpuMatched, truthOf, centerOf, null, out countMatched, out rounds));
                for (int j = 0; j < K; j++)
                {
                    centers[j].matched_X = gpuMatched[3 * j];
                    centers[j].matched_Y = gpuMatched[3 * j + 1];
                    centers[j].matched_Z = gpuMatched[3 * j + 2];
                    centers[j].isMatched = truthOf[j] >= 0;
                    if (truthOf[j] >= 0) { centers[j].matchNum = truthOf[j]; matchedID.Add(truthOf[j]); }
                }
                for (int i = 0; i < T; i++) if (centerOf[i] < 0) unmatchedTruths.Add(i);
            }
            else
            {
                for (int i = 0; i < T; i++) unmatchedTruths.Add(i);
            }
            this.toolStripStatusLabelCurrentPointCount.Text = "总共" + centers.Count + "个聚类质心，总共" + T + "个真值点，匹配" + countMatched + "个点";
            showMatchedLine(isShowUnmatchedCenterPts, isShowUnmatchedTruePts);
        }

        // In place of the bounding-box factors of showTruesAndCenters (FrmMain.cs:3046-3055): the ratio of the two extents
        // is the ratio of a window to the field when the scan sees part of the truths, and one false cluster at the edge
        // moves it for every point.  Here the scale is the k of the best similarity a pair of centroids and a pair of
        // truths agree on (vcp_register_sim), one factor for both axes.  bases = pairs of indices into centers.  Returns
        // false, with scale and tmp_X / tmp_Y untouched, when no base found a pair in [scaleMin, scaleMax].
        public bool ScaleCentersBySimilarity(int[] bases, double scaleMin, double scaleMax, bool mirror, double inlierDist)
        {
            int K = centers.Count, nb = bases.Length / 2;
            if (K < 2 || nb < 1) return false;
            double[] c = new double[3 * K];
            for (int j = 0; j < K; j++) { c[3 * j] = centers[j].X; c[3 * j + 1] = centers[j].Y; c[3 * j + 2] = 0.0; }
            double[] M16 = new double[16], k = new double[nb];
            int best;
            using (VcpNative.Lease lease = VcpNative.Rent())
                VcpNative.Check(lease, VcpNative.vcp_register_sim(lease.Ctx, c, K, TruthArray(), (int)truePointCloud.GetNumberOfPoints(),
                    bases, nb, scaleMin, scaleMax, mirror ? 1 : 0, 200, inlierDist, M16, out best, null, null, null, null, null, k));
            if (best < 0) return false;
            scale[0] = k[best];
            scale[1] = k[best];
            foreach (Point3D p in centers)
            {
                p.tmp_X = p.X * scale[0];
                p.tmp_Y = p.Y * scale[1];
            }
            return true;
        }

        // FrmMain.cs:3437-3467: nearest truth within the radius per raw point (the LINQ query :3452-3456)
        private void refreshClusList()
        {
            double clusterRadius;
            if (!double.TryParse(this.PtsInRegionTxt.Text, out clusterRadius))
            {
                MessageBox.Show("输入的文件格式有误，请重新输入");
                return;
            }
            isStartDrawCircle = true;
            foreach (ClusObj oj in clusList) oj.li.Clear();
            int n = rawData.Count, T = trues.Count;
            double[] mot = new double[2 * n], txy = new double[2 * T];
            int[] tid = new int[T], ids = new int[n];
            for (int i = 0; i < n; i++) { mot[2 * i] = rawData[i].motor_x; mot[2 * i + 1] = rawData[i].motor_y; }
            for (int s = 0; s < T; s++) { txy[2 * s] = trues[s].tmp_X; txy[2 * s + 1] = trues[s].tmp_Y; tid[s] = trues[s].clusterId; }
            long yedian = 0;
            if (n > 0)
                using (VcpNative.Lease lease = VcpNative.Rent())
                    VcpNative.Check(lease, VcpNative.vcp_assign_truths(lease.Ctx, mot, n, txy, tid, T, clusterRadius, ids, out yedian));
            for (int i = 0; i < n; i++) if (ids[i] != 0) clusList[ids[i] - 1].li.Add(rawData[i]);
            this.toolStripStatusLabelCurrentPointCount.Text = String.Format("当前聚类个数：{0}，有效点个数： {1}，野点个数： {2}", (clusList.Count(i => i.li.Count != 0)), rawData.Count - yedian, yedian);
            addCircles();
        }

        // FrmMain.cs:841-907.  The reference hands the centroids (tmp_X, tmp_Y, 0) -- Tools.ArrayList2PolyData type 1,
        // Tools.cs:696-703 -- and the truth points to VTK's closed vtkIterativeClosestPointTransform with RigidBody,
        // 100 iterations, StartByMatchingCentroidsOn and everything else at its defaults (:851-858).  vcp_icp_vtklike runs
        // that configuration (VTK 5.0 header: every ns/200-th source point is a landmark, closest target point per
        // landmark, rigid-body landmark fit per round); parity against VTK itself is unpinned (closed binary).
        // M receives the accumulated matrix like icp.GetMatrix() (:862); the display part is the reference's own, with a
        // plain vtkTransform carrying M in place of the icp object.
        void ICP()
        {
            ren = new vtk.vtkRenderer();
            vtk.vtkPolyData SourcePolydata = Tools.ArrayList2PolyData(1, this.centers, this.trueScale, this.centroidScale,
                this.scale, this.clock, this.clock_y, this.clock_x);
            vtk.vtkPolyData TargetPolydata = new vtk.vtkPolyData();
            TargetPolydata.SetPoints(truePointCloud);
            TargetPolydata.SetVerts(truePointVertices);

            int ns = centers.Count;
            double[] src = new double[3 * Math.Max(ns, 1)];
            for (int i = 0; i < ns; i++) { src[3 * i] = centers[i].tmp_X; src[3 * i + 1] = centers[i].tmp_Y; src[3 * i + 2] = 0.0; }
            double[] tgt = TruthArray();
            double[] m16 = new double[16];
            double meanDist; int iters;
            using (VcpNative.Lease lease = VcpNative.Rent())
                VcpNative.Check(lease, VcpNative.vcp_icp_vtklike(lease.Ctx, src, ns, tgt, tgt.Length / 3, 100, 200, 1, m16,
                    out meanDist, out iters));
            M = new vtk.vtkMatrix4x4();
            for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) M.SetElement(r, c, m16[4 * r + c]);
            Console.WriteLine("刚性变换矩阵为：" + M);
            ShowIcpSolution(SourcePolydata, TargetPolydata);
        }

        // ICP() from `angles` start rotations about z (and their mirror images: an unknown axis direction, the xdir / ydir
        // the user types at import, :912-913) instead of the centroid start alone -- the local minimum the reference lists
        // under "bugs known".  Same inputs as ICP(); the start whose result puts the most centroids within matchDistance
        // of a truth wins, and M is set the same way, so calMatchedCoords / RecorrectMatchingPtsByDistance run unchanged.
        void ICPMultiStart(int angles, bool mirror, double matchDistance)
        {
            ren = new vtk.vtkRenderer();
            vtk.vtkPolyData SourcePolydata = Tools.ArrayList2PolyData(1, this.centers, this.trueScale, this.centroidScale,
                this.scale, this.clock, this.clock_y, this.clock_x);
            vtk.vtkPolyData TargetPolydata = new vtk.vtkPolyData();
            TargetPolydata.SetPoints(truePointCloud);
            TargetPolydata.SetVerts(truePointVertices);

            int ns = centers.Count;
            double[] src = new double[3 * Math.Max(ns, 1)];
            for (int i = 0; i < ns; i++) { src[3 * i] = centers[i].tmp_X; src[3 * i + 1] = centers[i].tmp_Y; src[3 * i + 2] = 0.0; }
            double[] tgt = TruthArray();
            int poses = mirror ? 2 * angles : angles;
            double[] initR = null;  // null: the library's Rz(h * 2 pi / angles)
            if (mirror)
            {
                initR = new double[9 * poses];
                for (int h = 0; h < angles; h++)
                {
                    double t = h * (2.0 * Math.PI / angles), c = Math.Cos(t), s = Math.Sin(t);
                    double[] rz = { c, 0.0 - s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0 };
                    double[] rm = { c, s, 0.0, s, 0.0 - c, 0.0, 0.0, 0.0, 1.0 };  // Rz(t) * diag(1, -1, 1)
                    Array.Copy(rz, 0, initR, 9 * h, 9);
                    Array.Copy(rm, 0, initR, 9 * (angles + h), 9);
                }
            }
            double[] m16 = new double[16];
            int[] inliers = new int[Math.Max(poses, 1)];
            int best;
            using (VcpNative.Lease lease = VcpNative.Rent())
                VcpNative.Check(lease, VcpNative.vcp_icp_multistart(lease.Ctx, src, ns, tgt, tgt.Length / 3, poses, initR, null,
                    100, 200, matchDistance, m16, out best, null, null, inliers));
            M = new vtk.vtkMatrix4x4();
            for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) M.SetElement(r, c, m16[4 * r + c]);
            Console.WriteLine("刚性变换矩阵为：" + M + " (start " + best + " of " + poses + ", " + inliers[best] + " / " + ns + ")");
            ShowIcpSolution(SourcePolydata, TargetPolydata);
        }

        // ICPMultiStart() with a gate on the centroid-to-truth distance: false clusters the radius / aspect filter left in
        // (a wall beside the target field, clutter between targets) pull every round of ICP(); here round r leaves a
        // centroid out of the fit when its nearest truth is gates[r] or farther away, the gate shrinking geometrically
        // from gateStart (about the truths' spacing) to gateEnd (a few times the centroid noise) over the first 10 rounds
        // and held there.  A round with fewer than 3 centroids inside the gate changes nothing.  M is set as by ICP().
        void ICPGated(int angles, bool mirror, double gateStart, double gateEnd, double matchDistance)
        {
            ren = new vtk.vtkRenderer();
            vtk.vtkPolyData SourcePolydata = Tools.ArrayList2PolyData(1, this.centers, this.trueScale, this.centroidScale,
                this.scale, this.clock, this.clock_y, this.clock_x);
            vtk.vtkPolyData TargetPolydata = new vtk.vtkPolyData();
            TargetPolydata.SetPoints(truePointCloud);
            TargetPolydata.SetVerts(truePointVertices);

            int ns = centers.Count;
            double[] src = new double[3 * Math.Max(ns, 1)];
            for (int i = 0; i < ns; i++) { src[3 * i] = centers[i].tmp_X; src[3 * i + 1] = centers[i].tmp_Y; src[3 * i + 2] = 0.0; }
            double[] tgt = TruthArray();
            int poses = mirror ? 2 * angles : angles;
            double[] initR = null;  // null: the library's Rz(h * 2 pi / angles)
            if (mirror)
            {
                initR = new double[9 * poses];
                for (int h = 0; h < angles; h++)
                {
                    double t = h * (2.0 * Math.PI / angles), c = Math.Cos(t), s = Math.Sin(t);
                    double[] rz = { c, 0.0 - s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0 };
                    double[] rm = { c, s, 0.0, s, 0.0 - c, 0.0, 0.0, 0.0, 1.0 };  // Rz(t) * diag(1, -1, 1)
                    Array.Copy(rz, 0, initR, 9 * h, 9);
                    Array.Copy(rm, 0, initR, 9 * (angles + h), 9);
                }
            }
            const int steps = 10;
            double[] gates = new double[steps];
            for (int k = 0; k < steps; k++) gates[k] = gateStart * Math.Pow(gateEnd / gateStart, k / (steps - 1.0));
            gates[0] = gateStart;
            gates[steps - 1] = gateEnd;
            double[] m16 = new double[16];
            int[] inliers = new int[Math.Max(poses, 1)];
            long[] kept = new long[Math.Max(poses, 1)];
            int[] starved = new int[Math.Max(poses, 1)];
            int best;
            using (VcpNative.Lease lease = VcpNative.Rent())
                VcpNative.Check(lease, VcpNative.vcp_icp_gated(lease.Ctx, src, ns, tgt, tgt.Length / 3, poses, initR, null,
                    100, 200, gates, steps, 3, matchDistance, m16, out best, null, null, inliers, kept, starved));
            M = new vtk.vtkMatrix4x4();
            for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) M.SetElement(r, c, m16[4 * r + c]);
            Console.WriteLine("刚性变换矩阵为：" + M + " (start " + best + " of " + poses + ", " + inliers[best] + " / " + ns
                + ", " + kept[best] + " inside the gate, " + starved[best] + " starved rounds)");
            ShowIcpSolution(SourcePolydata, TargetPolydata);
        }

        // ICPMultiStart() where every round fits on a share of the centroids: the ceil(keepShare * count) of them that lie
        // closest to their nearest truth, the others left out of that round.  keepShare is the share of the centroids
        // expected to be real targets, min(1, visible * truths / centroids) -- known before any pose exists, and free of
        // the scan's unit, where ICPGated's two distances are not.  M is set as by ICP().
        void ICPTrimmed(int angles, bool mirror, double keepShare, double matchDistance)
        {
            ren = new vtk.vtkRenderer();
            vtk.vtkPolyData SourcePolydata = Tools.ArrayList2PolyData(1, this.centers, this.trueScale, this.centroidScale,
                this.scale, this.clock, this.clock_y, this.clock_x);
            vtk.vtkPolyData TargetPolydata = new vtk.vtkPolyData();
            TargetPolydata.SetPoints(truePointCloud);
            TargetPolydata.SetVerts(truePointVertices);

            int ns = centers.Count;
            double[] src = new double[3 * Math.Max(ns, 1)];
            for (int i = 0; i < ns; i++) { src[3 * i] = centers[i].tmp_X; src[3 * i + 1] = centers[i].tmp_Y; src[3 * i + 2] = 0.0; }
            double[] tgt = TruthArray();
            int poses = mirror ? 2 * angles : angles;
            double[] initR = null;  // null: the library's Rz(h * 2 pi / angles)
            if (mirror)
            {
                initR = new double[9 * poses];
                for (int h = 0; h < angles; h++)
                {
                    double t = h * (2.0 * Math.PI / angles), c = Math.Cos(t), s = Math.Sin(t);
                    double[] rz = { c, 0.0 - s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0 };
                    double[] rm = { c, s, 0.0, s, 0.0 - c, 0.0, 0.0, 0.0, 1.0 };  // Rz(t) * diag(1, -1, 1)
                    Array.Copy(rz, 0, initR, 9 * h, 9);
                    Array.Copy(rm, 0, initR, 9 * (angles + h), 9);
                }
            }
            double[] keep = { keepShare };
            double[] m16 = new double[16];
            int[] inliers = new int[Math.Max(poses, 1)];
            long[] kept = new long[Math.Max(poses, 1)];
            int[] starved = new int[Math.Max(poses, 1)];
            double[] trimDist = new double[Math.Max(poses, 1)];
            int best;
            using (VcpNative.Lease lease = VcpNative.Rent())
                VcpNative.Check(lease, VcpNative.vcp_icp_trimmed(lease.Ctx, src, ns, tgt, tgt.Length / 3, poses, initR, null,
                    100, 200, keep, 1, 3, matchDistance, m16, out best, null, null, inliers, kept, starved, trimDist));
            M = new vtk.vtkMatrix4x4();
            for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) M.SetElement(r, c, m16[4 * r + c]);
            Console.WriteLine("刚性变换矩阵为：" + M + " (start " + best + " of " + poses + ", " + inliers[best] + " / " + ns
                + ", " + kept[best] + " kept within " + trimDist[best] + ", " + starved[best] + " starved rounds)");
            ShowIcpSolution(SourcePolydata, TargetPolydata);
        }

        // ICPGated() for centroids whose unit is only roughly the truths' (vtkLandmarkTransform's Similarity mode, which
        // ICP() switches off at FrmMain.cs:854 because showTruesAndCenters scaled by the bounding boxes first): every round
        // also fits one isotropic scale from the centroids inside the gate.  The start is startScale times a rotation about
        // z (the bounding-box factor, or RegisterSimilarity's k); the rounds may change the scale by a factor within
        // [1 / maxRatio, maxRatio].  A start scale that is off by 2 % moves the edge of a 20 x 20 field by more than a
        // closed gate of 0.1, and ICPGated() then keeps only the middle of the field.  M is set as by ICP().
        void ICPSimilarity(int angles, double startScale, double maxRatio, double gateStart, double gateEnd, double matchDistance)
        {
            ren = new vtk.vtkRenderer();
            vtk.vtkPolyData SourcePolydata = Tools.ArrayList2PolyData(1, this.centers, this.trueScale, this.centroidScale,
                this.scale, this.clock, this.clock_y, this.clock_x);
            vtk.vtkPolyData TargetPolydata = new vtk.vtkPolyData();
            TargetPolydata.SetPoints(truePointCloud);
            TargetPolydata.SetVerts(truePointVertices);

            int ns = centers.Count;
            double[] src = new double[3 * Math.Max(ns, 1)];
            for (int i = 0; i < ns; i++) { src[3 * i] = centers[i].tmp_X; src[3 * i + 1] = centers[i].tmp_Y; src[3 * i + 2] = 0.0; }
            double[] tgt = TruthArray();
            int nt = tgt.Length / 3;
            // means for the start translation T0 = mean(truths) - R0 mean(centroids), R0 = startScale Rz
            double[] ms = new double[3], mt = new double[3];
            for (int i = 0; i < ns; i++) for (int c = 0; c < 3; c++) ms[c] += src[3 * i + c];
            for (int i = 0; i < nt; i++) for (int c = 0; c < 3; c++) mt[c] += tgt[3 * i + c];
            for (int c = 0; c < 3; c++) { ms[c] /= Math.Max(ns, 1); mt[c] /= Math.Max(nt, 1); }
            double[] initR = new double[9 * angles], initT = new double[3 * angles];
            for (int h = 0; h < angles; h++)
            {
                double t = h * (2.0 * Math.PI / angles), c = startScale * Math.Cos(t), s = startScale * Math.Sin(t);
                double[] r0 = { c, 0.0 - s, 0.0, s, c, 0.0, 0.0, 0.0, startScale };
                Array.Copy(r0, 0, initR, 9 * h, 9);
                for (int r = 0; r < 3; r++)
                    initT[3 * h + r] = mt[r] - (r0[3 * r] * ms[0] + r0[3 * r + 1] * ms[1] + r0[3 * r + 2] * ms[2]);
            }
            const int steps = 10;
            double[] gates = new double[steps];
            for (int k = 0; k < steps; k++) gates[k] = gateStart * Math.Pow(gateEnd / gateStart, k / (steps - 1.0));
            gates[0] = gateStart;
            gates[steps - 1] = gateEnd;
            double[] m16 = new double[16];
            int[] inliers = new int[Math.Max(angles, 1)];
            long[] kept = new long[Math.Max(angles, 1)];
            int[] starved = new int[Math.Max(angles, 1)];
            double[] ratio = new double[Math.Max(angles, 1)];
            int[] unscaled = new int[Math.Max(angles, 1)];
            int best;
            using (VcpNative.Lease lease = VcpNative.Rent())
                VcpNative.Check(lease, VcpNative.vcp_icp_sim(lease.Ctx, src, ns, tgt, nt, angles, initR, initT, 100, 200, gates,
                    steps, 3, 1.0 / maxRatio, maxRatio, matchDistance, m16, out best, null, null, inliers, kept, starved, ratio,
                    unscaled));
            M = new vtk.vtkMatrix4x4();
            for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) M.SetElement(r, c, m16[4 * r + c]);
            Console.WriteLine("相似变换矩阵为：" + M + " (start " + best + " of " + angles + ", " + inliers[best] + " / " + ns
                + ", " + kept[best] + " inside the gate, scale " + startScale * ratio[best] + " = start x " + ratio[best] + ", "
                + starved[best] + " starved and " + unscaled[best] + " unscaled rounds)");
            ShowIcpSolution(SourcePolydata, TargetPolydata);
        }

        // ICPGated() that fits the reference's OWN pose model: tmp_X = X * scale[0], tmp_Y = Y * scale[1], then a rigid
        // motion (showTruesAndCenters, FrmMain.cs:3046-3055, then ICP()).  The motor's two axes do not have the same gain, so
        // the two factors differ; the bounding boxes give them once, wrongly on a partial view or with one false cluster at
        // the edge.  Here every round fits both factors by least squares on the centroids inside the gate, beside the
        // rotation and the translation (vcp_icp_aniso).  The start is scale[0], scale[1] as they stand (the bounding-box
        // rule, or ScaleCentersBySimilarity's k in both); each may change by a factor within [1 / maxRatio, maxRatio].  The
        // RAW centroid coordinates go in.  On return scale[0], scale[1] and tmp_X, tmp_Y hold the fitted factors and M the
        // rigid part, so that M applied to (tmp_X, tmp_Y, 0) is the pose found -- what ICP() leaves behind.
        void ICPAnisotropic(int angles, double maxRatio, double gateStart, double gateEnd, double matchDistance)
        {
            ren = new vtk.vtkRenderer();
            int ns = centers.Count;
            double[] src = new double[3 * Math.Max(ns, 1)];
            for (int i = 0; i < ns; i++) { src[3 * i] = centers[i].X; src[3 * i + 1] = centers[i].Y; src[3 * i + 2] = 0.0; }
            double[] tgt = TruthArray();
            int nt = tgt.Length / 3;
            double[] initScale = new double[2 * angles];
            for (int h = 0; h < angles; h++) { initScale[2 * h] = scale[0]; initScale[2 * h + 1] = scale[1]; }
            const int steps = 10;
            double[] gates = new double[steps];
            for (int k = 0; k < steps; k++) gates[k] = gateStart * Math.Pow(gateEnd / gateStart, k / (steps - 1.0));
            gates[0] = gateStart;
            gates[steps - 1] = gateEnd;
            double[] m16 = new double[16];
            int[] inliers = new int[Math.Max(angles, 1)];
            long[] kept = new long[Math.Max(angles, 1)];
            int[] starved = new int[Math.Max(angles, 1)];
            double[] fitted = new double[2 * Math.Max(angles, 1)];
            int[] unscaled = new int[2 * Math.Max(angles, 1)];
            int best;
            // init_R null: the library's Rz(h * 2 pi / angles); init_T null: its centroid start under R diag(scale)
            using (VcpNative.Lease lease = VcpNative.Rent())
                VcpNative.Check(lease, VcpNative.vcp_icp_aniso(lease.Ctx, src, ns, tgt, nt, angles, null, null, initScale, 100, 200,
                    gates, steps, 3, 1.0 / maxRatio, maxRatio, matchDistance, m16, out best, null, null, inliers, kept, starved,
                    fitted, unscaled));
            scale[0] = fitted[2 * best];
            scale[1] = fitted[2 * best + 1];
            foreach (Point3D p in centers)
            {
                p.tmp_X = p.X * scale[0];
                p.tmp_Y = p.Y * scale[1];
            }
            // m16 holds [R diag(sx, sy, 1) | t]: the rigid part is its first two columns over the factors
            M = new vtk.vtkMatrix4x4();
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++)
                    M.SetElement(r, c, r < 3 && c < 2 ? m16[4 * r + c] / scale[c] : m16[4 * r + c]);
            vtk.vtkPolyData SourcePolydata = Tools.ArrayList2PolyData(1, this.centers, this.trueScale, this.centroidScale,
                this.scale, this.clock, this.clock_y, this.clock_x);
            vtk.vtkPolyData TargetPolydata = new vtk.vtkPolyData();
            TargetPolydata.SetPoints(truePointCloud);
            TargetPolydata.SetVerts(truePointVertices);
            Console.WriteLine("刚性变换矩阵为：" + M + " (start " + best + " of " + angles + ", " + inliers[best] + " / " + ns
                + ", " + kept[best] + " inside the gate, scale " + scale[0] + " x " + scale[1] + ", " + starved[best]
                + " starved rounds, " + unscaled[2 * best] + " / " + unscaled[2 * best + 1] + " rounds without an x / y scale)");
            ShowIcpSolution(SourcePolydata, TargetPolydata);
        }

        // ICPGated() where a truth takes one centroid per round: of the centroids whose nearest truth is the same one, only
        // the closest enters that round's fit.  A target makes one centroid; where DBSCAN split it, or a reflection or an
        // edge return left a second cluster beside it, the second lies inside any gate that admits the real centroids and
        // pulls ICPGated()'s pose by its offset times the ghosts' share.  M is set as by ICP().
        void ICPUnique(int angles, bool mirror, double gateStart, double gateEnd, double matchDistance)
        {
            ren = new vtk.vtkRenderer();
            vtk.vtkPolyData SourcePolydata = Tools.ArrayList2PolyData(1, this.centers, this.trueScale, this.centroidScale,
                this.scale, this.clock, this.clock_y, this.clock_x);
            vtk.vtkPolyData TargetPolydata = new vtk.vtkPolyData();
            TargetPolydata.SetPoints(truePointCloud);
            TargetPolydata.SetVerts(truePointVertices);

            int ns = centers.Count;
            double[] src = new double[3 * Math.Max(ns, 1)];
            for (int i = 0; i < ns; i++) { src[3 * i] = centers[i].tmp_X; src[3 * i + 1] = centers[i].tmp_Y; src[3 * i + 2] = 0.0; }
            double[] tgt = TruthArray();
            int poses = mirror ? 2 * angles : angles;
            double[] initR = null;  // null: the library's Rz(h * 2 pi / angles)
            if (mirror)
            {
                initR = new double[9 * poses];
                for (int h = 0; h < angles; h++)
                {
                    double t = h * (2.0 * Math.PI / angles), c = Math.Cos(t), s = Math.Sin(t);
                    double[] rz = { c, 0.0 - s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0 };
                    double[] rm = { c, s, 0.0, s, 0.0 - c, 0.0, 0.0, 0.0, 1.0 };  // Rz(t) * diag(1, -1, 1)
                    Array.Copy(rz, 0, initR, 9 * h, 9);
                    Array.Copy(rm, 0, initR, 9 * (angles + h), 9);
                }
            }
            const int steps = 10;
            double[] gates = new double[steps];
            for (int k = 0; k < steps; k++) gates[k] = gateStart * Math.Pow(gateEnd / gateStart, k / (steps - 1.0));
            gates[0] = gateStart;
            gates[steps - 1] = gateEnd;
            double[] m16 = new double[16];
            int[] inliers = new int[Math.Max(poses, 1)];
            long[] kept = new long[Math.Max(poses, 1)];
            int[] starved = new int[Math.Max(poses, 1)];
            long[] lost = new long[Math.Max(poses, 1)];
            int best;
            using (VcpNative.Lease lease = VcpNative.Rent())
                VcpNative.Check(lease, VcpNative.vcp_icp_unique(lease.Ctx, src, ns, tgt, tgt.Length / 3, poses, initR, null,
                    100, 200, gates, steps, 3, matchDistance, m16, out best, null, null, inliers, kept, starved, lost));
            M = new vtk.vtkMatrix4x4();
            for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) M.SetElement(r, c, m16[4 * r + c]);
            Console.WriteLine("刚性变换矩阵为：" + M + " (start " + best + " of " + poses + ", " + inliers[best] + " / " + ns
                + ", " + kept[best] + " kept, " + lost[best] + " lost their truth to a closer centroid, " + starved[best]
                + " starved rounds)");
            ShowIcpSolution(SourcePolydata, TargetPolydata);
        }

        // the display part of FrmMain.cs:863-906: the centroids moved by M next to the truths
        void ShowIcpSolution(vtk.vtkPolyData SourcePolydata, vtk.vtkPolyData TargetPolydata)
        {
            vtk.vtkTransform solved = new vtk.vtkTransform();
            solved.SetMatrix(M);
            vtk.vtkTransformPolyDataFilter icpTransformFilter = new vtk.vtkTransformPolyDataFilter();
            icpTransformFilter.SetInput(SourcePolydata);
            icpTransformFilter.SetTransform(solved);
            icpTransformFilter.Update();
            vtk.vtkPolyDataMapper targetMapper = new vtk.vtkPolyDataMapper();
            targetMapper.SetInputConnection(TargetPolydata.GetProducerPort());
            vtk.vtkActor targetActor = new vtk.vtkActor();
            targetActor.SetMapper(targetMapper);
            targetActor.GetProperty().SetColor(0, 1, 0);
            targetActor.GetProperty().SetPointSize(4);
            vtk.vtkPolyDataMapper solutionMapper = new vtk.vtkPolyDataMapper();
            solutionMapper.SetInputConnection(icpTransformFilter.GetOutputPort());
            vtk.vtkActor solutionActor = new vtk.vtkActor();
            solutionActor.SetMapper(solutionMapper);
            solutionActor.GetProperty().SetColor(0, 0, 1);
            solutionActor.GetProperty().SetPointSize(3);
            ren.AddActor(targetActor);
            ren.AddActor(solutionActor);
            vtkControl.GetRenderWindow().AddRenderer(ren);
            SourcePolydata.FastDelete();
            TargetPolydata.FastDelete();
        }

        // The row loop of AddFolder for scan files (FrmMain.cs:991-1090, typpe 1 = remove duplicates, 2 = keep them).
        // AddFolder keeps its file / tree-view code; per file it now only PARSES (FileMap.ReadFile + Split('\t') +
        // Convert.ToDouble, :1005-1008, or the xls cells :996-1001) into rows = (motor_x, motor_y, Distance) triples and
        // collects them, then calls this once for all files of the folder:
        //     List<double> rows = new List<double>(); List<int> rowPath = new List<int>();
        //     foreach file: foreach parsed line: rows.Add(mx); rows.Add(my); rows.Add(dist); rowPath.Add(pathList.Count);
        //                   pathList.Add(file);
        //     duplicatNum += AddScanRows(rows.ToArray(), rowPath.ToArray(), typpe, xdir, ydir);
        // One call = one native conversion: the Distance filter (:1011), the spherical conversion (:1025-1062) and, for
        // typpe 1, the duplicate test against every EARLIER kept row (:1063-1068: rawData.FindAll over the whole list, so
        // duplicates across files count too) run on the GPU (hash table instead of the O(n^2) FindAll); rows already in
        // rawData from an earlier AddFolder are passed in front so that they take part in the test.  Fixed-point files
        // (typpe 3 / 4) keep the reference's loop: a handful of rows per file.
        int AddScanRows(double[] rows, int[] rowPath, int typpe, int xdir, int ydir)
        {
            int nNew = rowPath.Length;
            int nOld = (typpe == 1) ? rawData.Count : 0;   // earlier points take part in the duplicate test only
            int n = nOld + nNew;
            if (nNew == 0) return 0;
            double[] all = new double[3 * n];
            for (int i = 0; i < nOld; i++) { all[3 * i] = rawData[i].motor_x; all[3 * i + 1] = rawData[i].motor_y; all[3 * i + 2] = rawData[i].Distance; }
            Array.Copy(rows, 0, all, 3 * nOld, 3 * nNew);
            double[] xyz = new double[3 * n];
            byte[] state = new byte[n];
            long kept, dup;
            using (VcpNative.Lease lease = VcpNative.Rent())
                VcpNative.Check(lease, VcpNative.vcp_import_convert(lease.Ctx, all, n, this.x_angle, this.y_angle, xdir, ydir,
                    typpe == 1 ? 1 : 0, xyz, state, out kept, out dup));
            int duplicates = 0;
            for (int i = nOld; i < n; i++)
            {
                if (state[i] == 0) continue;                  // Distance == 0 or > 1000 (:1011)
                if (state[i] == 2) { duplicates++; continue; }  // equals an earlier kept row (:1065-1068)
                Point3D point = new Point3D();
                point.motor_x = all[3 * i]; point.motor_y = all[3 * i + 1]; point.Distance = all[3 * i + 2];
                point.pathId = rowPath[i - nOld];
                point.ifShown = true;
                point.isClassed = false;
                point.clusterId = 0;
                point.X = xyz[3 * i]; point.Y = xyz[3 * i + 1]; point.Z = xyz[3 * i + 2];
                rawData.Add(point);
            }
            return duplicates;
        }

        // FrmMain.cs:1905-1920: filterID = the clusters whose circumscribed circle exceeds `radius`.  The circles of
        // clusters 1..clusterSum (Tools.getCircles: clusID = position + 1) go to vcp_cluster_filter as one array each;
        // a cluster without a circle (<= 3 points) is never listed.
        public void FilterClustersByRadius(double radius)
        {
            FilterClusters(radius, double.PositiveInfinity);
            this.toolStripStatusLabel2.Text = "超过阈值半径聚类数：" + filterID.Count;
            showCircle(circles, 2, rawData, centers);
        }

        // The README's second criterion ("length / width ratio", on the circumscribed rectangle): filterID = the clusters
        // whose longer side exceeds `aspect` times the shorter one.  No counterpart body in FrmMain.cs.
        public void FilterClustersByAspect(double aspect)
        {
            FilterClusters(double.PositiveInfinity, aspect);
            this.toolStripStatusLabel2.Text = "超过阈值长宽比聚类数：" + filterID.Count;
        }

        void FilterClusters(double maxRadius, double maxAspect)
        {
            filterID.Clear();
            int K = clusterSum;
            if (K <= 0) return;
            double[] rad = new double[K], rlen = new double[2 * K];
            byte[] valid = new byte[K], rvalid = new byte[K], filtered = new byte[K];
            foreach (Point2D c in circles) { rad[c.clusID - 1] = c.radius; valid[c.clusID - 1] = 1; }
            bool aspect = !double.IsPositiveInfinity(maxAspect) && !double.IsNaN(maxAspect);
            if (aspect)
                foreach (Tools.Rect2D r in Tools.getRectangles(clusList, false))
                { rlen[2 * (r.clusID - 1)] = r.len0; rlen[2 * (r.clusID - 1) + 1] = r.len1; rvalid[r.clusID - 1] = 1; }
            int nf; long nk;
            using (VcpNative.Lease lease = VcpNative.Rent())
                VcpNative.Check(lease, VcpNative.vcp_cluster_filter(lease.Ctx, new int[0], 0, K, rad, valid, aspect ? rlen : null,
                    aspect ? rvalid : null, maxRadius, maxAspect, filtered, null, null, out nf, out nk));
            for (int j = 0; j < K; j++) if (filtered[j] != 0) filterID.Add(j + 1);
        }

        // Beside RejectPtsByDistanceFromFixed (FrmMain.cs:1759-1764), which confirms the one band of Distance the
        // SureDistanceFilter dialog applied to every file (Tools.FilterByDistance_FixedPoint, Tools.cs:438-461): here every
        // file gets its own band, |Distance - median| <= max(c * MAD, floor) (vcp_cluster_mad), so that targets at
        // different ranges are cleaned alike.  Sets isFilterByDistance the way the dialog does, then removes the marked
        // points like Tools.cleanDataByDistance2 (Tools.cs:259-262); Tools.getFixedPtsCentroid follows as before.
        // Returns the number of points removed.  An empty clusList removes nothing.
        public long RejectPtsByDistanceRobust(double c, double floor)
        {
            int K = clusList == null ? 0 : clusList.Count, n = 0;
            for (int i = 0; i < K; i++) n += clusList[i].li.Count;
            if (K == 0 || n == 0) return 0;
            double[] dist = new double[n], med = new double[K], mad = new double[K], thr = new double[K];
            int[] group = new int[n];
            byte[] reject = new byte[n];
            long[] kept = new long[K];
            int t = 0;
            for (int i = 0; i < K; i++)
                foreach (Point3D p in clusList[i].li) { dist[t] = p.Distance; group[t] = i + 1; t++; }
            long rejected;
            using (VcpNative.Lease lease = VcpNative.Rent())
                VcpNative.Check(lease, VcpNative.vcp_cluster_mad(lease.Ctx, dist, 1, group, n, K, c, floor, med, mad, thr,
                    reject, kept, out rejected));
            t = 0;
            for (int i = 0; i < K; i++)
                foreach (Point3D p in clusList[i].li) p.isFilterByDistance = reject[t++] != 0;
            for (int i = 0; i < K; i++)
                clusList[i].li.RemoveAll(delegate(Point3D p) { return p.isFilterByDistance; });
            this.FixedPointMatchingToolStripMenuItem.Enabled = true;
            return rejected;
        }

        // FrmMain.cs:3743-3746
        public void removePointByRadius()
        {
            Tools.removeFilterPointFromClustering(ref rawData, filterID);
            Tools.removeFilterPointFromClustering(ref centers, filterID);
        }
    }
}
