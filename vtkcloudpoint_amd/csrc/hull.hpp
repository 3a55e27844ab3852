// hull.hpp -- the per-cluster shape pass shared by mcc.hip (vcp_mcc) and shapes.hip (vcp_cluster_shapes): the convex
// hull of Geometry.MakeConvexHull, built ONCE per cluster in LDS, then the minimal bounding circle of
// Geometry.FindMinimalBoundingCircle and -- for vcp_cluster_shapes only -- the minimum-area bounding rectangle and the
// hull's list positions.
//
// Reference: BaseClass/Tools.cs:394-409 (one circle per cluster with more than 3 points) and
// BaseClass/Geometry.cs:247-319 (MakeConvexHull :122-208 = gift wrapping on the pseudo-angle of AngleValue
// :220-246; then the smallest circle through 2 or 3 hull points that encloses the hull, first found on ties;
// FindCircle :340-372 via FindIntersection :373-432).  HullCull (:83-120) culls nothing but NaN points: the
// Rectangle2D it compares against never gets Left/Right/Top/Bottom assigned (DataModel.cs:191-208).
//
// One 256-thread workgroup per cluster.  The members of a cluster are first brought together in list order
// (stable rocPRIM radix sort by label).  Every choice the C# makes sequentially ("first in the list wins") is
// an argmin over (value, list position), so the parallel reductions reproduce it exactly; the arithmetic is
// binary64 without FMA contraction, sqrt and division correctly rounded: results are bit-identical to the oracle.
//
// Behind the reference's wrap and search stand two rules of this library's own, both made of
// exact comparisons of the same expressions on host and device.  Covering: when rounding leaves no pair or triple
// that encloses the hull (points on a common circle), the search runs again and a candidate counts with its distance
// to the farthest hull point.  Insertion: when a member lies strictly farther from the centre than every hull point,
// the wrap closed early (a cluster collinear up to rounding); the farthest such member joins the list and the search
// runs again.  Both are rare; the common path pays one strided pass over the members and two block reductions.
//
// The rectangle is defined in include/vcp.h (no C# body stands behind it: Polygon.cs has no caller): hull edges over
// the lanes, each lane walking the hull in LDS (every lane reads the same address: a broadcast), then one
// (area, edge) lexicographic minimum.
#pragma once
#include <cmath>

#include "vcp_ctx.hpp"
#include "wave.hpp"

namespace {
constexpr int MT = 256;
constexpr int HMAX = 2048;  // hull points kept in LDS (32 KB); a larger hull is reported as VCP_ERR_TOO_LARGE
constexpr double DMAX = 1.7976931348623157e308;

__global__ __launch_bounds__(MT) void k_mcc_gather(const double* __restrict__ xy, const uint32_t* __restrict__ idx,
                                                  int64_t m, double* __restrict__ cxy) {
  int64_t t = (int64_t)blockIdx.x * MT + threadIdx.x;
  if (t >= m) return;
  *reinterpret_cast<double2*>(cxy + 2 * t) = *reinterpret_cast<const double2*>(xy + 2 * (int64_t)idx[t]);
}

__device__ __forceinline__ double angle_value(double x1, double y1, double x2, double y2) {  // Geometry.cs:220-246
  double dx = x2 - x1, ax = fabs(dx), dy = y2 - y1, ay = fabs(dy), t;
  if (ax + ay == 0)
    t = 40.0;  // 360f / 9f
  else
    t = dy / (ax + ay);
  if (dx < 0)
    t = 2 - t;
  else if (dy < 0)
    t = 4 + t;
  return t * 90;
}

struct Key {  // (value, value2, position): lexicographic minimum = "first in the list among the smallest"
  double a, b;
  uint32_t p;
};
__device__ __forceinline__ bool key_less(const Key& x, const Key& y) {
  if (x.a < y.a) return true;
  if (x.a > y.a) return false;
  if (x.b < y.b) return true;
  if (x.b > y.b) return false;
  return x.p < y.p;
}
__device__ __forceinline__ Key key_shfl(const Key& k, int d) {
  Key r;
  r.a = __shfl_xor(k.a, d, 64);
  r.b = __shfl_xor(k.b, d, 64);
  r.p = (uint32_t)__shfl_xor((int)k.p, d, 64);
  return r;
}
// block-wide lexicographic minimum; every thread gets the result
__device__ __forceinline__ Key block_min(Key k, Key* sm /*[MT/64]*/) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    Key o = key_shfl(k, d);
    if (key_less(o, k)) k = o;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = k;
  __syncthreads();
  Key r = sm[0];
#pragma unroll
  for (int w = 1; w < MT / 64; w++)
    if (key_less(sm[w], r)) r = sm[w];
  return r;
}

struct Best {  // (radius^2, sequence number of the candidate in the C#'s loop order)
  double r2;
  unsigned long long seq;
};

__device__ __forceinline__ bool encloses(double cx, double cy, double r2, const double2* hull, int h, int s1, int s2,
                                         int s3) {  // Geometry.cs:322-337
  for (int i = 0; i < h; i++)
    if (i != s1 && i != s2 && i != s3) {
      double dx = cx - hull[i].x, dy = cy - hull[i].y;
      if (dx * dx + dy * dy > r2) return false;
    }
  return true;
}

__device__ __forceinline__ void find_circle(double2 a, double2 b, double2 c, double* cx, double* cy, double* r2) {
  // Geometry.cs:340-372 with FindIntersection :373-406
  double x1 = (b.x + a.x) / 2, y1 = (b.y + a.y) / 2, dy1 = b.x - a.x, dx1 = -(b.y - a.y);
  double x2 = (c.x + b.x) / 2, y2 = (c.y + b.y) / 2, dy2 = c.x - b.x, dx2 = -(c.y - b.y);
  double p2x = x1 + dx1, p2y = y1 + dy1, p4x = x2 + dx2, p4y = y2 + dy2;
  double dx12 = p2x - x1, dy12 = p2y - y1, dx34 = p4x - x2, dy34 = p4y - y2;
  double den = dy12 * dx34 - dx12 * dy34;
  double t1 = ((x1 - x2) * dy34 + (y2 - y1) * dx34) / den;
  *cx = x1 + dx12 * t1;
  *cy = y1 + dy12 * t1;
  double dx = *cx - a.x, dy = *cy - a.y;
  *r2 = dx * dx + dy * dy;
}

// One candidate of the search: it replaces `mine` when it is smaller (earlier in the C#'s loop order on ties) and
// encloses the list.  cover: its value is the squared distance to the farthest point of the list, not its radius^2.
__device__ __forceinline__ void candidate(Best& mine, double cx, double cy, double tr2, unsigned long long seq,
                                          const double2* hull, int h, int s1, int s2, int s3, bool cover) {
  double val = tr2;
  if (cover) {
    val = -INFINITY;
    for (int i = 0; i < h; i++) {
      const double dx = cx - hull[i].x, dy = cy - hull[i].y, d = dx * dx + dy * dy;
      if (!(d == d)) return;
      val = d > val ? d : val;
    }
  }
  if (!((val < mine.r2 || (val == mine.r2 && seq < mine.seq)) && val < DMAX)) return;
  if (!cover && !encloses(cx, cy, tr2, hull, h, s1, s2, s3)) return;
  mine.r2 = val;
  mine.seq = seq;
}

// The bounding rectangle with one side on hull edge i (include/vcp.h, "cluster shapes"): extents of the hull in the
// edge's frame, scaled by the squared edge length.  false = the edge is no candidate.
// mem != null (a cluster on which the insertion rule fired: the hull is incomplete): the extents are taken over the
// cnt members that HullCull keeps instead of over the hull.
struct EdgeBox {
  double ax, ay, dx, dy, L2, u0, u1, v0, v1, area;
};
__device__ __forceinline__ bool edge_box(const double2* hull, int h, int i, const double2* __restrict__ mem, uint32_t cnt,
                                         EdgeBox* e) {
  const double2 a = hull[i], b = hull[i + 1 == h ? 0 : i + 1];
  const double dx = b.x - a.x, dy = b.y - a.y, L2 = dx * dx + dy * dy;
  if (!(L2 > 0 && L2 < INFINITY)) return false;
  double u0 = INFINITY, u1 = -INFINITY, v0 = INFINITY, v1 = -INFINITY;
  bool nan = false;
  auto take = [&](const double2 p) {
    const double rx = p.x - a.x, ry = p.y - a.y;
    const double u = rx * dx + ry * dy, v = ry * dx - rx * dy;
    nan |= !(u == u) || !(v == v);
    u0 = u < u0 ? u : u0;
    u1 = u > u1 ? u : u1;
    v0 = v < v0 ? v : v0;
    v1 = v > v1 ? v : v1;
  };
  if (!mem) {
    for (int j = 0; j < h; j++) take(hull[j]);
  } else {
    for (uint32_t t = 0; t < cnt; t++) {
      const double2 p = mem[t];
      if (!(p.x != p.x && p.y != p.y)) take(p);
    }
  }
  if (nan) return false;
  // a zero extreme is +0 whichever of -0 / +0 the hull point produced
  e->u0 = u0 + 0.0, e->u1 = u1 + 0.0, e->v0 = v0 + 0.0, e->v1 = v1 + 0.0;
  e->ax = a.x, e->ay = a.y, e->dx = dx, e->dy = dy, e->L2 = L2;
  e->area = ((e->u1 - e->u0) * (e->v1 - e->v0)) / L2;
  return e->area < INFINITY;
}

// what vcp_cluster_shapes adds to the circle (every output pointer may be null)
struct ShapeOut {
  const uint32_t* sorted;  // [m] point of every member slot (vcp_group_by_label)
  uint32_t* hull_pt;       // [m] the hull of cluster k as points of the caller's array, at segstart[k]
  double* rect_xy;
  double* rect_len;
  int32_t* rect_edge;
  uint8_t* rect_valid;
};

__device__ __forceinline__ void no_rectangle(const ShapeOut& so, int k, double x, double y) {
  if (so.rect_valid) so.rect_valid[k - 1] = 0;
  if (so.rect_edge) so.rect_edge[k - 1] = -1;
  if (so.rect_len) so.rect_len[2 * (k - 1)] = so.rect_len[2 * (k - 1) + 1] = 0;
  if (so.rect_xy)
    for (int c = 0; c < 4; c++) {
      so.rect_xy[8 * (k - 1) + 2 * c] = x;
      so.rect_xy[8 * (k - 1) + 2 * c + 1] = y;
    }
}

// The body of one workgroup = one cluster k = blockIdx.x + 1.
// segstart[k] = first member slot of cluster k (k = 1..K; slot range of label 0 precedes them)
template <bool SHAPES>
__device__ __forceinline__ void cluster_fit(const double* __restrict__ cxy, const uint32_t* __restrict__ segstart,
                                            const uint32_t* __restrict__ counts, uint8_t* __restrict__ removed,
                                            double* __restrict__ centers, double* __restrict__ radius,
                                            uint8_t* __restrict__ valid, int32_t* __restrict__ hull_n,
                                            const ShapeOut& so) {
  const int k = blockIdx.x + 1;
  const uint32_t cnt = counts[k];
  const int tid = threadIdx.x;
  if (cnt <= 3) {  // Tools.cs:400
    if (tid == 0) {
      valid[k - 1] = 0;
      radius[k - 1] = 0;
      centers[2 * (k - 1)] = centers[2 * (k - 1) + 1] = 0;
      if (hull_n) hull_n[k - 1] = 0;
      if constexpr (SHAPES) no_rectangle(so, k, 0, 0);
    }
    return;
  }
  const double2* pts = reinterpret_cast<const double2*>(cxy) + segstart[k];
  uint8_t* rem = removed + segstart[k];
  __shared__ double2 hull[HMAX];
  __shared__ Key smk[MT / 64];
  __shared__ unsigned s_alive[MT / 64];

  // HullCull: only NaN coordinates fail every comparison and get dropped
  unsigned alive_local = 0;
  for (uint32_t t = tid; t < cnt; t += MT) {
    double2 p = pts[t];
    bool keep = !(p.x != p.x && p.y != p.y);  // `x <= L || x >= R || y <= T || y >= B` with L=R=T=B=0: false only for NaN,NaN
    rem[t] = keep ? 0 : 1;
    alive_local += keep;
  }
  {
    const unsigned v = wave_all<WaveAdd>(alive_local);
    __syncthreads();
    if ((tid & 63) == 0) s_alive[tid >> 6] = v;
    __syncthreads();
  }
  unsigned alive = 0;
  for (int w = 0; w < MT / 64; w++) alive += s_alive[w];
  if (alive == 0) {  // points[0] of an empty list: the C# throws; not reachable with finite input
    if (tid == 0) {
      valid[k - 1] = 3;
      if constexpr (SHAPES) hull_n[k - 1] = 0;
    }
    return;
  }
  // Geometry.cs:129-150: smallest y, then smallest x, first in the list
  Key kk{DMAX, DMAX, 0xFFFFFFFFu};
  for (uint32_t t = tid; t < cnt; t += MT)
    if (!rem[t]) {
      Key c{pts[t].y, pts[t].x, t};
      if (key_less(c, kk)) kk = c;
    }
  kk = block_min(kk, smk);
  int h = 0;
  if (tid == 0) {
    hull[0] = pts[kk.p];
    if constexpr (SHAPES)  // a hull never has more points than its cluster: h <= cnt slots from segstart[k]
      if (so.hull_pt) so.hull_pt[segstart[k]] = so.sorted[segstart[k] + kk.p];
    rem[kk.p] = 1;
  }
  h = 1;
  alive--;
  __syncthreads();
  double sweep = 0;
  bool overflow = false;
  while (alive > 0) {
    const double X = hull[h - 1].x, Y = hull[h - 1].y;
    // smallest pseudo-angle >= sweep (strictly below 3600), first in the list; and the first live point
    Key best{3600.0, 0.0, 0xFFFFFFFFu};
    Key first{0.0, 0.0, 0xFFFFFFFFu};  // a = b = 0 so that only the position orders it
    for (uint32_t t = tid; t < cnt; t += MT)
      if (!rem[t]) {
        if (t < first.p) first.p = t;
        double ta = angle_value(X, Y, pts[t].x, pts[t].y);
        if (ta >= sweep) {
          Key c{ta, 0.0, t};
          if (key_less(c, best)) best = c;
        }
      }
    best = block_min(best, smk);
    first = block_min(first, smk);
    uint32_t bp = best.p;
    double best_angle = best.a;
    if (bp == 0xFFFFFFFFu) {  // nobody qualified: best_pt stays points[0], best_angle stays 3600 (:168-169)
      bp = first.p;
      best_angle = 3600;
    }
    const double first_angle = angle_value(X, Y, hull[0].x, hull[0].y);
    if (first_angle >= sweep && best_angle >= first_angle) break;  // :190-195
    if (h >= HMAX) {
      overflow = true;
      break;
    }
    __syncthreads();
    if (tid == 0) {
      hull[h] = pts[bp];
      if constexpr (SHAPES)
        if (so.hull_pt) so.hull_pt[segstart[k] + h] = so.sorted[segstart[k] + bp];
      rem[bp] = 1;
    }
    h++;
    alive--;
    sweep = best_angle;
    __syncthreads();
  }
  __syncthreads();
  if (overflow) {
    if (tid == 0) {
      valid[k - 1] = 2;
      if (hull_n) hull_n[k - 1] = h;
    }
    return;
  }
  // S = hull[0 .. hs): the wrap's hull, then the members that the insertion rule adds
  int hs = h;
  bool cover = false;  // the plain search found nothing: candidates count with their reach over S
  bool fired = false;  // the insertion rule added a member
  __shared__ unsigned long long s_seq;
  __shared__ double s_fit[3];  // centre and radius of the current circle
  for (;;) {
    // Geometry.cs:260-312: pairs, then triples; the winner is the smallest (radius^2, loop position)
    Best mine{DMAX, ~0ull};
    const unsigned long long H = (unsigned long long)hs;
    for (int i = 0; i < hs - 1; i++)
      for (int j = i + 1 + tid; j < hs; j += MT) {
        const double tcx = (hull[i].x + hull[j].x) / 2.0, tcy = (hull[i].y + hull[j].y) / 2.0;
        const double dx = tcx - hull[i].x, dy = tcy - hull[i].y;
        candidate(mine, tcx, tcy, dx * dx + dy * dy, (unsigned long long)i * H + (unsigned long long)j, hull, hs, i, j, -1,
                  cover);
      }
    for (int i = 0; i < hs - 2; i++)
      for (int j = i + 1; j < hs - 1; j++)
        for (int kq = j + 1 + tid; kq < hs; kq += MT) {
          double tcx, tcy, tr2;
          find_circle(hull[i], hull[j], hull[kq], &tcx, &tcy, &tr2);
          candidate(mine, tcx, tcy, tr2, H * H + ((unsigned long long)i * H + (unsigned long long)j) * H + (unsigned long long)kq,
                    hull, hs, i, j, kq, cover);
        }
    // seq is 64-bit: reduce in two steps -- first the smallest r2, then the smallest seq among its holders
    const Key r2min = block_min(Key{mine.r2, 0.0, 0u}, smk);
    if (tid == 0) s_seq = ~0ull;
    __syncthreads();
    if (mine.r2 == r2min.a && mine.seq != ~0ull) atomicMin(&s_seq, mine.seq);
    __syncthreads();
    const unsigned long long seq = s_seq;
    const bool found = seq != ~0ull && r2min.a < DMAX;
    if (!found && !cover && hs > 2) {  // rounding left no triple that encloses: points on a common circle
      cover = true;
      continue;
    }
    if (tid == 0) {
      double cx = pts[0].x, cy = pts[0].y, rad = 0;  // best_center = points[0] of the ORIGINAL list (:254-257)
      if (found) {
        if (seq < H * H) {
          const int i = (int)(seq / H), j = (int)(seq % H);
          cx = (hull[i].x + hull[j].x) / 2.0;
          cy = (hull[i].y + hull[j].y) / 2.0;
        } else {
          const unsigned long long q = seq - H * H;
          const int kq = (int)(q % H), j = (int)((q / H) % H), i = (int)(q / (H * H));
          double r2;
          find_circle(hull[i], hull[j], hull[kq], &cx, &cy, &r2);
        }
        rad = sqrt(r2min.a);
      }
      s_fit[0] = cx, s_fit[1] = cy, s_fit[2] = rad;
    }
    __syncthreads();
    // the insertion rule: a member strictly farther from the centre than every point of S joins S
    const double cx = s_fit[0], cy = s_fit[1];
    double reach = -INFINITY;  // the farthest point of S; +inf once a distance is NaN, so that nothing is farther
    for (int i = tid; i < hs; i += MT) {
      const double dx = cx - hull[i].x, dy = cy - hull[i].y, d = dx * dx + dy * dy;
      reach = !(d == d) ? INFINITY : (d > reach ? d : reach);
    }
    Key far{INFINITY, 0.0, 0xFFFFFFFFu};  // (-distance^2, position): the farthest member, the first in the list on ties
    for (uint32_t t = tid; t < cnt; t += MT) {
      const double dx = cx - pts[t].x, dy = cy - pts[t].y, d = dx * dx + dy * dy;
      if (d == d) {
        Key c{-d, 0.0, t};
        if (key_less(c, far)) far = c;
      }
    }
    const Key rs = block_min(Key{-reach, 0.0, 0u}, smk);
    far = block_min(far, smk);
    if (!(far.p != 0xFFFFFFFFu && -far.a > -rs.a)) break;
    if (hs >= HMAX) {
      overflow = true;
      break;
    }
    if (tid == 0) hull[hs] = pts[far.p];
    hs++;
    fired = true;
    cover = false;
    __syncthreads();
  }
  if (overflow) {
    if (tid == 0) {
      valid[k - 1] = 2;
      if (hull_n) hull_n[k - 1] = h;
    }
    return;
  }
  if (tid == 0) {
    centers[2 * (k - 1)] = s_fit[0];
    centers[2 * (k - 1) + 1] = s_fit[1];
    radius[k - 1] = s_fit[2];
    valid[k - 1] = 1;
    if (hull_n) hull_n[k - 1] = h;
  }
  if constexpr (SHAPES) {
    // the smallest (area, edge): one edge per lane and round, the hull walked out of LDS
    // (the edges are the wrap's; where the insertion rule fired, their extents are taken over the members)
    const double2* mem = fired ? pts : nullptr;
    Key rk{INFINITY, 0.0, 0xFFFFFFFFu};
    EdgeBox e;
    for (int i = tid; i < h; i += MT)
      if (edge_box(hull, h, i, mem, cnt, &e)) {
        Key c{e.area, 0.0, (uint32_t)i};
        if (key_less(c, rk)) rk = c;
      }
    rk = block_min(rk, smk);
    if (tid == 0) {
      if (rk.p == 0xFFFFFFFFu) {
        no_rectangle(so, k, hull[0].x, hull[0].y);
      } else {
        edge_box(hull, h, (int)rk.p, mem, cnt, &e);
        if (so.rect_valid) so.rect_valid[k - 1] = 1;
        if (so.rect_edge) so.rect_edge[k - 1] = (int32_t)rk.p;
        if (so.rect_len) {
          const double L = sqrt(e.L2);
          so.rect_len[2 * (k - 1)] = (e.u1 - e.u0) / L;
          so.rect_len[2 * (k - 1) + 1] = (e.v1 - e.v0) / L;
        }
        if (so.rect_xy) {
          const double us[4] = {e.u0, e.u1, e.u1, e.u0}, vs[4] = {e.v0, e.v0, e.v1, e.v1};
#pragma unroll
          for (int c = 0; c < 4; c++) {
            so.rect_xy[8 * (k - 1) + 2 * c] = e.ax + (us[c] * e.dx - vs[c] * e.dy) / e.L2;
            so.rect_xy[8 * (k - 1) + 2 * c + 1] = e.ay + (us[c] * e.dy + vs[c] * e.dx) / e.L2;
          }
        }
      }
    }
  }
}

// the circle alone (vcp_mcc; vcp_cluster_shapes without rectangle and hull outputs)
// segstart[k] = first member slot of cluster k (k = 1..K; slot range of label 0 precedes them)
__global__ __launch_bounds__(MT) void k_mcc(const double* __restrict__ cxy, const uint32_t* __restrict__ segstart,
                                           const uint32_t* __restrict__ counts, uint8_t* __restrict__ removed,
                                           double* __restrict__ centers, double* __restrict__ radius,
                                           uint8_t* __restrict__ valid, int32_t* __restrict__ hull_n) {
  cluster_fit<false>(cxy, segstart, counts, removed, centers, radius, valid, hull_n, ShapeOut{});
}

}  // namespace
