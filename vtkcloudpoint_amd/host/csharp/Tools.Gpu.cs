// Tools.Gpu.cs -- the Tools statics on the hot path, as a drop-in: add `partial` to the declaration in
// vtkPointCloud/BaseClass/Tools.cs:11 (`partial class Tools`), delete the originals named below from that file
// (same names, same signatures, same in-place effects) and add this file to the project.  Nothing else in Tools.cs
// changes; the callers (FrmMain.cs:1533, Clustering.cs:125-181, SureDistanceFilter.cs:74, FrmMain.cs:1539-1540) stay
// as they are.
using System;
using System.Collections.Generic;
using System.Linq;

namespace vtkPointCloud
{
    partial class Tools
    {
        // Tools.GetClusList, Tools.cs:162-195
        public static void GetClusList(List<Point3D> rawData, List<Point3D> centers, List<Point3D> centers2D,
                                       List<ClusObj> clusList, List<int> idList)
        {
            int n = rawData.Count, K = clusList.Count;
            double[] xyz = new double[3 * n], mot = new double[2 * n];
            int[] lab = new int[n];
            for (int i = 0; i < n; i++)
            {
                Point3D p = rawData[i];
                xyz[3 * i] = p.X; xyz[3 * i + 1] = p.Y; xyz[3 * i + 2] = p.Z;
                mot[2 * i] = p.motor_x; mot[2 * i + 1] = p.motor_y;
                lab[i] = p.clusterId;
                if (p.clusterId != 0) clusList[p.clusterId - 1].li.Add(p);
            }
            if (K == 0 || n == 0) return;
            double[] c3 = new double[3 * K], c2 = new double[2 * K];
            long[] cnt = new long[K];
            using (VcpNative.Lease c = VcpNative.Rent())
                VcpNative.Check(c, VcpNative.vcp_centroids(c.Ctx, xyz, mot, lab, n, K, c3, c2, cnt));
            for (int k = 0; k < K; k++)
            {
                if (cnt[k] == 0) continue;
                centers.Add(new Point3D(c3[3 * k], c3[3 * k + 1], c3[3 * k + 2], clusList[k].clusId, true));
                centers2D.Add(new Point3D(c2[2 * k], c2[2 * k + 1], 0, clusList[k].clusId, true));
            }
        }

        // Tools.MergeIDByDistance, Tools.cs:580-621
        public static Dictionary<int, int> MergeIDByDistance(List<Point3D> centers, double thre)
        {
            Dictionary<int, int> dick = new Dictionary<int, int>();
            int K = centers.Count;
            if (K == 0) return dick;
            double[] cxy = new double[2 * K];
            int[] ids = new int[K], mapTo = new int[K];
            for (int k = 0; k < K; k++)
            {
                Point3D p = centers[k];
                p.IDBeforeMerge = p.clusterId; p.motor_x = p.X; p.motor_y = p.Y; p.clusterId = 0;
                cxy[2 * k] = p.X; cxy[2 * k + 1] = p.Y; ids[k] = p.IDBeforeMerge;
            }
            int mergeCount;
            using (VcpNative.Lease c = VcpNative.Rent())
                VcpNative.Check(c, VcpNative.vcp_merge_centroids(c.Ctx, cxy, ids, K, thre, mapTo, out mergeCount));
            for (int k = 0; k < K; k++) if (mapTo[k] != 0) dick.Add(ids[k], mapTo[k]);
            return dick;
        }

        // Tools.refreshCensAndClusByDictionary, Tools.cs:521-572 (caller Clustering.cs:125-181): the points of every list
        // whose id is a key of dic move to the END of list dic[id] (in clusList order), the merged lists go, the rest
        // is renumbered 1..K' by ascending id and every centroid is recomputed.  List surgery stays here (it is the
        // caller-visible structure); relabelling + renumbering + the K' x 5 means are one native call.
        static public void refreshCensAndClusByDictionary(Dictionary<int, int> dic, List<ClusObj> clusList,
                                                          ref List<Point3D> centers, ref List<Point3D> centers2D)
        {
            int K0 = clusList.Count;
            // like the C#, a target is addressed by POSITION dic[id] - 1 (clusList[k].clusId == k + 1 on entry, Tools.cs:531)
            foreach (ClusObj ob in clusList.ToArray())
                if (dic.ContainsKey(ob.clusId)) clusList[dic[ob.clusId] - 1].li.AddRange(ob.li);
            clusList.RemoveAll(delegate(ClusObj o) { return dic.ContainsKey(o.clusId); });
            clusList.Sort(delegate(ClusObj a, ClusObj b) { return a.clusId.CompareTo(b.clusId); });   // ids are distinct
            int n = 0, K = 0;
            foreach (ClusObj ob in clusList) { n += ob.li.Count; K = Math.Max(K, ob.clusId); }
            K = Math.Max(K, K0);
            double[] xyz = new double[3 * Math.Max(n, 1)], mot = new double[2 * Math.Max(n, 1)];
            int[] lab = new int[Math.Max(n, 1)], mapById = new int[Math.Max(K, 1)];   // the moves are done: identity map
            int t = 0;
            foreach (ClusObj ob in clusList)
                foreach (Point3D p in ob.li)
                {
                    xyz[3 * t] = p.X; xyz[3 * t + 1] = p.Y; xyz[3 * t + 2] = p.Z;
                    mot[2 * t] = p.motor_x; mot[2 * t + 1] = p.motor_y;
                    lab[t++] = ob.clusId;
                }
            int newK = 0;
            double[] c3 = new double[3 * Math.Max(K, 1)], c2 = new double[2 * Math.Max(K, 1)];
            long[] cnt = new long[Math.Max(K, 1)];
            if (n > 0)
                using (VcpNative.Lease c = VcpNative.Rent())
                    VcpNative.Check(c, VcpNative.vcp_refresh_by_dictionary(c.Ctx, xyz, mot, lab, n, K, mapById, out newK, c3, c2, cnt));
            // surviving ids in ascending order take 1..K' (:551-560).  A surviving list WITHOUT points keeps its number in
            // the C# too (idForMerge counts lists, the native call counts ids that still have points): number by position
            int idForMerge = 0, k = 0;
            t = 0;
            foreach (ClusObj ob in clusList)
            {
                ob.clusId = ++idForMerge;
                foreach (Point3D pp in ob.li) pp.clusterId = idForMerge;
                if (ob.li.Count == 0)
                {   // obj.li.Average on an empty list throws InvalidOperationException in the C# (:563)
                    throw new InvalidOperationException("Sequence contains no elements");
                }
                centers.Add(new Point3D(c3[3 * k], c3[3 * k + 1], c3[3 * k + 2], ob.clusId, true));
                centers2D.Add(new Point3D(c2[2 * k], c2[2 * k + 1], 0, ob.clusId, true));
                k++;
            }
            Console.WriteLine("keys中包含" + dic.Count + "质心有" + centers.Count);
        }

        // Tools.getFixedPtsCentroid, Tools.cs:78-111 (caller SureDistanceFilter.cs:74)
        static public List<Point3D> getFixedPtsCentroid(List<ClusObj> clusList, bool isIgnoreDuplication)
        {
            List<Point3D> scanCen = new List<Point3D>();
            int K = clusList.Count, n = 0;
            for (int i = 0; i < K; i++) n += clusList[i].li.Count;
            if (K == 0) return scanCen;
            double[] xyz = new double[3 * Math.Max(n, 1)];
            int[] group = new int[Math.Max(n, 1)], cid = new int[Math.Max(n, 1)], cnt = new int[Math.Max(n, 1)];
            int t = 0;
            for (int i = 0; i < K; i++)
                foreach (Point3D p in clusList[i].li)
                {
                    xyz[3 * t] = p.X; xyz[3 * t + 1] = p.Y; xyz[3 * t + 2] = p.Z;
                    group[t] = i + 1; cid[t] = p.clusterId; cnt[t] = p.ptsCount; t++;
                }
            double[] c3 = new double[3 * K];
            long[] inside = new long[K];
            // an empty list: VCP_ERR_INDEX, where the C# throws ArgumentOutOfRangeException at li[0] (:106)
            using (VcpNative.Lease c = VcpNative.Rent())
                VcpNative.Check(c, VcpNative.vcp_centroids_weighted(c.Ctx, xyz, group, cid, cnt, n, K,
                isIgnoreDuplication ? 1 : 0, c3, inside));
            for (int i = 0; i < K; i++)
            {
                Point3D tmp = new Point3D();
                tmp.X = c3[3 * i]; tmp.Y = c3[3 * i + 1]; tmp.Z = c3[3 * i + 2];
                tmp.pointName = clusList[i].li[0].pointName;
                tmp.ifShown = true;
                scanCen.Add(tmp);
            }
            return scanCen;
        }

        // Tools.getCircles, Tools.cs:394-409 (Geometry.FindMinimalBoundingCircle, Geometry.cs:247-319)
        static public List<Point2D> getCircles(List<ClusObj> clusList, bool is3D)
        {
            List<Point2D> circles = new List<Point2D>();
            int K = clusList.Count, n = 0;
            for (int j = 0; j < K; j++) n += clusList[j].li.Count;
            if (K == 0 || n == 0) return circles;
            double[] xy = new double[2 * n];
            int[] lab = new int[n];
            int t = 0;
            for (int j = 0; j < K; j++)
                foreach (Point3D p in clusList[j].li)
                {   // FindMinimalBoundingCircle reads X,Y for the 3-D view, motor_x,motor_y for the 2-D one
                    xy[2 * t] = is3D ? p.X : p.motor_x; xy[2 * t + 1] = is3D ? p.Y : p.motor_y; lab[t] = j + 1; t++;
                }
            double[] cen = new double[2 * K], rad = new double[K];
            byte[] valid = new byte[K];
            using (VcpNative.Lease c = VcpNative.Rent())
                VcpNative.Check(c, VcpNative.vcp_mcc(c.Ctx, xy, lab, null, n, n, K, cen, rad, valid, null));
            for (int j = 0; j < K; j++)
            {
                if (valid[j] == 0) continue;   // li.Count <= 3 (:400)
                Point2D c = new Point2D(cen[2 * j], cen[2 * j + 1]);
                c.radius = rad[j];
                c.clusID = j + 1;
                circles.Add(c);
            }
            return circles;
        }

        // The circumscribed rectangle the reference's README pairs with the circle (no body in Tools.cs; vcp.h, "cluster
        // shapes"): one Rect2D per cluster that has one -- more than 3 points that are not all equal -- from the same
        // pass that gives getCircles its circles.  clusID = position + 1, like getCircles.
        public class Rect2D
        {
            public int clusID;
            public double len0, len1;              // the side on the hull edge first
            public double[] corners = new double[8];
            public double Aspect { get { return Math.Max(len0, len1) / Math.Min(len0, len1); } }   // +inf on a line
        }

        static public List<Rect2D> getRectangles(List<ClusObj> clusList, bool is3D)
        {
            List<Rect2D> rects = new List<Rect2D>();
            int K = clusList.Count, n = 0;
            for (int j = 0; j < K; j++) n += clusList[j].li.Count;
            if (K == 0 || n == 0) return rects;
            double[] xy = new double[2 * n];
            int[] lab = new int[n];
            int t = 0;
            for (int j = 0; j < K; j++)
                foreach (Point3D p in clusList[j].li)
                {
                    xy[2 * t] = is3D ? p.X : p.motor_x; xy[2 * t + 1] = is3D ? p.Y : p.motor_y; lab[t] = j + 1; t++;
                }
            double[] cen = new double[2 * K], rad = new double[K], rxy = new double[8 * K], rlen = new double[2 * K];
            byte[] valid = new byte[K], rvalid = new byte[K];
            using (VcpNative.Lease c = VcpNative.Rent())
                VcpNative.Check(c, VcpNative.vcp_cluster_shapes(c.Ctx, xy, lab, null, n, n, K, cen, rad, valid, null, rxy, rlen,
                    null, rvalid, null, null));
            for (int j = 0; j < K; j++)
            {
                if (rvalid[j] == 0) continue;
                Rect2D r = new Rect2D();
                r.clusID = j + 1; r.len0 = rlen[2 * j]; r.len1 = rlen[2 * j + 1];
                Array.Copy(rxy, 8 * j, r.corners, 0, 8);
                rects.Add(r);
            }
            return rects;
        }

        // The moment ellipse of one cluster (vcp.h, "per-cluster covariance"): centre, the semi-axes 2 sigma (the longer
        // first), the unit direction of the longer one, flatness and tilt (0 and 1 for the 2-D view).  clusID = position + 1.
        public class Ellipse2D
        {
            public int clusID;
            public double[] center, axis;          // 2 entries, or 3 with is3D
            public double a, b, flatness, tilt;
            public double Aspect { get { return a / b; } }   // +inf on a line
        }

        // Beside getCircles / getRectangles: one ellipse per cluster of two or more points with finite moments, of
        // (X, Y, Z) with is3D, else of (motor_x, motor_y).  No hull: no limit on the size of a cluster.
        static public List<Ellipse2D> getEllipses(List<ClusObj> clusList, bool is3D)
        {
            List<Ellipse2D> ells = new List<Ellipse2D>();
            int K = clusList.Count, n = 0, d = is3D ? 3 : 2;
            for (int j = 0; j < K; j++) n += clusList[j].li.Count;
            if (K == 0 || n == 0) return ells;
            double[] pts = new double[d * n];
            int[] lab = new int[n];
            int t = 0;
            for (int j = 0; j < K; j++)
                foreach (Point3D p in clusList[j].li)
                {
                    if (is3D) { pts[3 * t] = p.X; pts[3 * t + 1] = p.Y; pts[3 * t + 2] = p.Z; }
                    else { pts[2 * t] = p.motor_x; pts[2 * t + 1] = p.motor_y; }
                    lab[t] = j + 1; t++;
                }
            double[] mean = new double[d * K], evec = new double[d * d * K], shape = new double[4 * K];
            byte[] valid = new byte[K];
            using (VcpNative.Lease c = VcpNative.Rent())
                VcpNative.Check(c, VcpNative.vcp_cluster_moments(c.Ctx, pts, d, d, lab, null, n, K, mean, null, null, evec, shape,
                    valid, null));
            for (int j = 0; j < K; j++)
            {
                if (valid[j] == 0) continue;
                Ellipse2D e = new Ellipse2D();
                e.clusID = j + 1; e.center = new double[d]; e.axis = new double[d];
                Array.Copy(mean, d * j, e.center, 0, d);
                Array.Copy(evec, d * d * j, e.axis, 0, d);
                e.a = 2.0 * shape[4 * j]; e.b = 2.0 * shape[4 * j + 1]; e.flatness = shape[4 * j + 2]; e.tilt = shape[4 * j + 3];
                ells.Add(e);
            }
            return ells;
        }

        // The least-squares sphere (is3D) or circle of one cluster (vcp.h, "per-cluster least-squares sphere"): the centre the
        // returns lie around (their mean sits 2/3 of a radius in front of it), the radius, the rms of the residuals and cap,
        // which says how one-sided the returns are (2/3 for a sphere seen from afar).  clusID = position + 1.
        public class Sphere
        {
            public int clusID;
            public double[] center;                // 2 entries, or 3 with is3D
            public double radius, rms, cap;
        }

        // Beside getCircles / getRectangles / getEllipses: one Sphere per cluster with a valid fit, of (X, Y, Z) with is3D,
        // else of (motor_x, motor_y).  radius 0 fits the radius; a value > 0 fixes it to the known target radius.
        static public List<Sphere> getSpheres(List<ClusObj> clusList, bool is3D, double radius)
        {
            List<Sphere> sph = new List<Sphere>();
            int K = clusList.Count, n = 0, d = is3D ? 3 : 2;
            for (int j = 0; j < K; j++) n += clusList[j].li.Count;
            if (K == 0 || n == 0) return sph;
            double[] pts = new double[d * n];
            int[] lab = new int[n];
            int t = 0;
            for (int j = 0; j < K; j++)
                foreach (Point3D p in clusList[j].li)
                {
                    if (is3D) { pts[3 * t] = p.X; pts[3 * t + 1] = p.Y; pts[3 * t + 2] = p.Z; }
                    else { pts[2 * t] = p.motor_x; pts[2 * t + 1] = p.motor_y; }
                    lab[t] = j + 1; t++;
                }
            double[] centre = new double[d * K], rad = new double[K], rms = new double[K], cap = new double[K];
            byte[] valid = new byte[K];
            using (VcpNative.Lease c = VcpNative.Rent())
                VcpNative.Check(c, VcpNative.vcp_cluster_spheres(c.Ctx, pts, d, d, lab, null, n, K, radius, 12, centre, rad, rms,
                    cap, null, null, valid, null));
            for (int j = 0; j < K; j++)
            {
                if (valid[j] == 0) continue;
                Sphere s = new Sphere();
                s.clusID = j + 1; s.center = new double[d];
                Array.Copy(centre, d * j, s.center, 0, d);
                s.radius = rad[j]; s.rms = rms[j]; s.cap = cap[j];
                sph.Add(s);
            }
            return sph;
        }

        // Tools.removeFilterPointFromClustering, Tools.cs:70-74: the stable RemoveAll, with the membership test of
        // filterID.Contains done once per listed id on the GPU side of vcp_cluster_filter.  Any int may be listed, 0 (the
        // noise points) and negative ids too, as Contains takes them; the arrays are as long as the list, not as its largest id
        static public void removeFilterPointFromClustering(ref List<Point3D> dataSet, List<int> filterID)
        {
            if (filterID.Count == 0) return;
            int n = dataSet.Count;
            if (n == 0) return;
            // the listed ids, each once, ascending: the r-th of them is cluster r + 1 of radius 1 against max_radius 0
            List<int> ids = new List<int>(filterID);
            ids.Sort();
            int K = 0;
            for (int r = 0; r < ids.Count; r++) if (r == 0 || ids[r] != ids[r - 1]) ids[K++] = ids[r];
            ids.RemoveRange(K, ids.Count - K);
            double[] rad = new double[K];
            byte[] valid = new byte[K], filtered = new byte[K];
            for (int r = 0; r < K; r++) { rad[r] = 1.0; valid[r] = 1; }
            int[] lab = new int[n], kept = new int[n];
            for (int i = 0; i < n; i++) { int r = ids.BinarySearch(dataSet[i].clusterId); lab[i] = r >= 0 ? r + 1 : 0; }
            int nf; long nk;
            using (VcpNative.Lease c = VcpNative.Rent())
                VcpNative.Check(c, VcpNative.vcp_cluster_filter(c.Ctx, lab, n, K, rad, valid, null, null, 0.0, double.PositiveInfinity,
                    filtered, null, kept, out nf, out nk));
            List<Point3D> outp = new List<Point3D>((int)nk);
            for (long t = 0; t < nk; t++) outp.Add(dataSet[kept[t]]);
            dataSet.Clear();
            dataSet.AddRange(outp);   // RemoveAll mutates the list the caller holds
        }

        // MainForm.getClusterFromMotor + DoWork3 + the labelling half of CompleteWork3
        // (FrmMain.cs:1214-1291, :1340-1361, :1442-1520) as one blocking call; returns clusForMerge.
        // partitionOnXY: the twin getClusterFromList (:1136-1213), whose rectangles are cut on (X, Y).
        // VcpNative.Devices = { 0, 1, ..., 7 } spreads the per-block step over those GPUs (one process, vcp_dbscan_blocks_multi).
        public static List<Point3D> ClusterBlocks(List<Point3D> rawData, double tr, int pts, int ptsInCell,
                                                  bool partitionOnXY, out int clusterAmount)
        {
            int n = rawData.Count;
            double[] mot = new double[2 * n];
            double[] key = partitionOnXY ? new double[2 * n] : null;
            for (int i = 0; i < n; i++)
            {
                mot[2 * i] = rawData[i].motor_x; mot[2 * i + 1] = rawData[i].motor_y;
                if (partitionOnXY) { key[2 * i] = rawData[i].X; key[2 * i + 1] = rawData[i].Y; }
            }
            int[] lab = new int[n], blk = new int[n];
            long[] order = new long[Math.Max(n, 1)];
            long m, ev; int rows, cols, kept, del;
            if (VcpNative.Devices.Length > 1)
            {   // several GPUs: the per-block DBImproved calls (StartCode on pool threads, FrmMain.cs:1356-1359) are split over
                // VcpNative.Devices by contiguous block ranges; same results, bit for bit
                lock (VcpNative.MultiLock)
                    VcpNative.CheckMulti(VcpNative.vcp_dbscan_blocks_multi(VcpNative.Multi, key, mot, n, tr, pts, ptsInCell, 3,
                        lab, blk, order, out m, out rows, out cols, out kept, out del, out clusterAmount, out ev));
            }
            else
            {
                using (VcpNative.Lease c = VcpNative.Rent(VcpNative.Devices.Length == 1 ? VcpNative.Devices[0] : VcpNative.Device))
                    VcpNative.Check(c, VcpNative.vcp_dbscan_blocks_keyed(c.Ctx, key, mot, n, tr, pts, ptsInCell, 3, lab, blk,
                        order, out m, out rows, out cols, out kept, out del, out clusterAmount, out ev));
            }
            for (int i = 0; i < n; i++) { rawData[i].clusterId = lab[i]; rawData[i].isClassed = lab[i] != 0; }
            List<Point3D> clusForMerge = new List<Point3D>((int)m);
            for (long t = 0; t < m; t++) clusForMerge.Add(rawData[(int)order[t]]);
            return clusForMerge;
        }

        // k-distance of every point for DBImproved with minPts = minPts (L1 on motor_x / motor_y, what the shipped
        // DBImproved measures): kd[i] <= eps exactly when the point is a core point at eps (vcp.h: vcp_kdist)
        public static double[] KDistance(List<Point3D> rawData, int minPts)
        {
            int n = rawData.Count;
            double[] mot = new double[2 * n], kd = new double[n];
            for (int i = 0; i < n; i++) { mot[2 * i] = rawData[i].motor_x; mot[2 * i + 1] = rawData[i].motor_y; }
            if (n == 0) return kd;
            using (VcpNative.Lease c = VcpNative.Rent())
                VcpNative.Check(c, VcpNative.vcp_kdist(c.Ctx, mot, n, 2, VcpNative.VCP_L1_2D, minPts, kd, null));
            return kd;
        }

        // A HEURISTIC eps for minPts: the knee of the sorted k-distance curve (vtkcloudpoint_amd/kdist.py: eps_from_curve)
        // -- finite values sorted, the top (1 - topQuantile) dropped, the rest mapped onto [0,1]^2, the value at the
        // first maximum of x - y.
        public static double SuggestEps(List<Point3D> rawData, int minPts, double topQuantile = 0.99)
        {
            double[] kd = KDistance(rawData, minPts);
            List<double> v = new List<double>(kd.Length);
            foreach (double d in kd) if (!double.IsNaN(d) && !double.IsInfinity(d)) v.Add(d);
            if (v.Count == 0) return double.NaN;
            v.Sort();
            double q = Math.Min(Math.Max(topQuantile, 0.0), 1.0);
            int m = (int)Math.Ceiling(q * (v.Count - 1)) + 1;
            double lo = v[0], hi = v[m - 1];
            if (m == 1 || !(hi > lo)) return lo;
            int best = 0;
            double bestGap = double.NegativeInfinity;
            for (int i = 0; i < m; i++)
            {
                double gap = (double)i / (m - 1) - (v[i] - lo) / (hi - lo);
                if (gap > bestGap) { bestGap = gap; best = i; }
            }
            return v[best];
        }

        // eps from the number of targets, not from a knee: the widest range [lo, hi) of eps <= epsMax on which
        // DBImproved(eps, minPts) finds exactly `target` clusters (vcp.h: vcp_eps_tree; vtkcloudpoint_amd/epstree.py:
        // eps_for_clusters).  clusters(eps) = #{kdist <= eps} - #{merge_w <= eps}; equal widths go to the lower lo; a
        // range that reaches epsMax includes it.  null when the count never occurs.  L1 on motor_x / motor_y.
        public static double[] EpsForClusters(List<Point3D> rawData, int minPts, double epsMax, int target)
        {
            int n = rawData.Count;
            if (n == 0) return null;
            double[] mot = new double[2 * n], kd = new double[n], mw = new double[Math.Max(n - 1, 1)];
            for (int i = 0; i < n; i++) { mot[2 * i] = rawData[i].motor_x; mot[2 * i + 1] = rawData[i].motor_y; }
            long m;
            int rounds;
            using (VcpNative.Lease c = VcpNative.Rent())
                VcpNative.Check(c, VcpNative.vcp_eps_tree(c.Ctx, mot, n, 2, VcpNative.VCP_L1_2D, minPts, epsMax, 0, kd, null,
                    out m, mw, null, null, out rounds));
            List<double> cores = new List<double>(n);
            foreach (double d in kd) if (d <= epsMax) cores.Add(d);
            cores.Sort();
            // the breakpoints, ascending: 0, every k-distance and every merge weight (both lists are sorted)
            List<double> br = new List<double>(cores.Count + (int)m + 1);
            br.Add(0.0);
            int a = 0, b = 0;
            while (a < cores.Count || b < m)
            {
                double v = b >= m || (a < cores.Count && cores[a] <= mw[b]) ? cores[a++] : mw[b++];
                if (v > br[br.Count - 1]) br.Add(v);
            }
            double[] bestIv = null;
            double lo = 0.0;
            bool open = false;
            a = 0; b = 0;
            for (int i = 0; i <= br.Count; i++)
            {
                bool ok = false;
                if (i < br.Count)
                {
                    while (a < cores.Count && cores[a] <= br[i]) a++;
                    while (b < m && mw[b] <= br[i]) b++;
                    ok = a - b == target;
                }
                if (ok && !open) { lo = br[i]; open = true; }
                if (!ok && open)
                {
                    double hi = i < br.Count ? br[i] : epsMax;
                    if (bestIv == null || hi - lo > bestIv[1] - bestIv[0]) bestIv = new double[] { lo, hi };
                    open = false;
                }
            }
            return bestIv;
        }

        // ---- the exports: one call builds the file's bytes (vcp.h: vcp_format_rows) -------------------------------------
        // The text of `[clusterId TAB] motor_x TAB motor_y TAB Distance` lines, "F<bit>", "\r\n": what the WriteLine loops
        // below wrote.  null when a value is outside what the device formats (a NaN, an infinity, 1e15 and more): the
        // caller then runs the original loop.  "F<bit>" of .NET 3.5 rounds a 15-digit expansion, the library the exact
        // binary value: the bytes agree on values read from text with at most `bit` decimals and 15 significant digits
        // (INTEGRATION.md).
        static byte[] FormatPoints(List<Point3D> pts, bool withId, int bit)
        {
            int n = pts.Count;
            if (n == 0) return new byte[0];
            double[] a = new double[n], b = new double[n], d = new double[n];
            int[] id = withId ? new int[n] : null;
            for (int i = 0; i < n; i++)
            {
                Point3D p = pts[i];
                a[i] = p.motor_x; b[i] = p.motor_y; d[i] = p.Distance;
                if (withId) id[i] = p.clusterId;
            }
            long[] err = new long[2];
            ulong nbytes;
            using (VcpNative.Lease c = VcpNative.Rent())
            {
                int rc = VcpNative.vcp_format_rows(c.Ctx, id, a, 1, b, 1, d, 1, null, n, n, bit, 1, null, 0, out nbytes, err);
                if (rc == -8) return null;
                VcpNative.Check(c, rc);
                byte[] text = new byte[nbytes];
                VcpNative.Check(c, VcpNative.vcp_format_rows(c.Ctx, id, a, 1, b, 1, d, 1, null, n, n, bit, 1, text, nbytes,
                    out nbytes, err));
                return text;
            }
        }

        // The write loop of Tools.cleanDataByDistance (Tools.cs:229-244, after the dialog): replace the StreamWriter block
        // by `Tools.WriteScanPoints(saveFile1.FileName, rawData, bit); skipRecru = false;`
        public static void WriteScanPoints(string path, List<Point3D> rawData, int bit)
        {
            byte[] text = FormatPoints(rawData, false, bit);
            if (text != null) { System.IO.File.WriteAllBytes(path, text); return; }
            using (System.IO.StreamWriter ssw = new System.IO.StreamWriter(path, false))
                foreach (Point3D p3d in rawData)
                    ssw.WriteLine(p3d.motor_x.ToString("F" + bit) + "\t" + p3d.motor_y.ToString("F" + bit) + "\t" + p3d.Distance.ToString("F" + bit));
        }

        // The write loop of Tools.cleanDataByDistance2 (Tools.cs:289-306): every li in list order, no id column
        public static void WriteFixedPoints(string path, List<ClusObj> clusList, int bit)
        {
            List<Point3D> all = new List<Point3D>();
            for (int i = 0; i < clusList.Count; i++) all.AddRange(clusList[i].li);
            WriteScanPoints(path, all, bit);
        }

        // Tools.exportClustersPointsFile, Tools.cs:364-387 (x_angle and y_angle are unused there as well)
        static public void exportClustersPointsFile(List<ClusObj> clusList, int bit, double x_angle, double y_angle, string ss)
        {
            List<Point3D> all = new List<Point3D>();
            for (int j = 0; j < clusList.Count; j++) all.AddRange(clusList[j].li);
            byte[] text = FormatPoints(all, true, bit);
            if (text != null) { System.IO.File.WriteAllBytes(ss, text); return; }
            using (System.IO.StreamWriter sw = new System.IO.StreamWriter(ss, false))
                foreach (Point3D p3d in all)
                    sw.WriteLine(p3d.clusterId + "\t" + p3d.motor_x.ToString("F" + bit) + "\t" + p3d.motor_y.ToString("F" + bit) + "\t" + p3d.Distance.ToString("F" + bit));
        }
    }
}
