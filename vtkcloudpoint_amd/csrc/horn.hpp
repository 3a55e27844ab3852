// horn.hpp -- Horn's unit-quaternion closed form, the solve of an ICP round (icp.hip): horn() for the rigid step,
// horn_sim() for the similarity step, horn_aniso() for the anisotropic one.  Host and device: same code, same rounding
// (vcp_selftest_horn, vcp_selftest_horn_sim and vcp_selftest_horn_aniso run it on the host).  Internal linkage, as when
// it was part of icp.hip.
#pragma once
#include <cmath>

namespace {

// cyclic Jacobi sweeps on a symmetric 4x4 (independent of the oracle's max-pivot variant).  Every index is a
// compile-time constant after unrolling, so on the device A and V live in registers (dynamic indexing would put
// them in scratch memory and make the single solving thread several times slower).
template <int P, int Q>
__host__ __device__ inline void jrot(double (&A)[4][4], double (&V)[4][4]) {
  if (A[P][Q] == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * A[P][Q]);
  const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double akp = A[k][P], akq = A[k][Q];
    A[k][P] = c * akp - s * akq;
    A[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double apk = A[P][k], aqk = A[Q][k];
    A[P][k] = c * apk - s * aqk;
    A[Q][k] = s * apk + c * aqk;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq;
    V[k][Q] = s * vkp + c * vkq;
  }
}

// A = V0^T Q V0 and V = V0 on entry (V0 = identity for a cold start): on return the columns of V are eigenvectors of Q
__host__ __device__ inline void jacobi4(double (&A)[4][4], double (&V)[4][4]) {
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0.0, diag = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      diag += A[i][i] * A[i][i];
#pragma unroll
      for (int j = i + 1; j < 4; j++) off += A[i][j] * A[i][j];
    }
    if (off <= 1e-34 * (diag + off) || off == 0.0) break;
    // three rounds of two rotations in DISJOINT planes: the angle of the second reads nothing the first one writes, so
    // the two chains of divisions and square roots overlap in the single lane that runs this
    jrot<0, 1>(A, V);
    jrot<2, 3>(A, V);
    jrot<0, 2>(A, V);
    jrot<1, 3>(A, V);
    jrot<0, 3>(A, V);
    jrot<1, 2>(A, V);
  }
}

// Vst [16]: the eigenvector basis of the previous round (row major), or NULL.  Consecutive rounds of an ICP solve
// nearly the same 4x4 problem, so the sweeps start from the previous basis (A = V^T Q V is then almost diagonal: one
// or two sweeps instead of six or seven -- the Jacobi chain is what bounds k_icp_step); the basis found is stored back.
// A basis that is not finite or has drifted from orthonormal (first round, failed round) is replaced by the identity.
__host__ __device__ inline bool horn(const double s[16], long long nd, double R1[9], double T1[3], double* Vst) {
  const double N = (double)nd;
  double Q[4][4], V[4][4];
  if (Vst) {  // read first: on the device the loads then fly while the divisions below run
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) V[i][j] = Vst[4 * i + j];
  }
  double muP[3], muY[3], m[3][3];
  for (int a = 0; a < 3; a++) {
    muP[a] = s[a] / N;
    muY[a] = s[3 + a] / N;
  }
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) m[r][c] = s[6 + 3 * r + c] / N - muP[r] * muY[c];
  const double tr = m[0][0] + m[1][1] + m[2][2];
  const double delta[3] = {m[1][2] - m[2][1], m[2][0] - m[0][2], m[0][1] - m[1][0]};
  Q[0][0] = tr;
  for (int i = 0; i < 3; i++) {
    Q[0][i + 1] = Q[i + 1][0] = delta[i];
    for (int j = 0; j < 3; j++) Q[i + 1][j + 1] = m[i][j] + m[j][i] - (i == j ? tr : 0.0);
  }
  // Q goes into the sweeps divided by the power of two that brings its largest entry into [0.5, 1): jacobi4's stop test
  // squares the entries, and beyond about 2^+-256 the squares overflow or flush to zero, which ended the sweeps before
  // the first rotation with "solved".  The division is exact and R1 depends on the eigenvectors alone, so nothing
  // changes where the squares were in range.  A non-finite entry (non-finite sums, or sums that overflow here) fails the
  // solve: an infinite off-diagonal entry passed the same stop test.  Tested per entry: fmax would drop a NaN.  The
  // verdict is returned at the end, not here: a branch at this point keeps the device compiler from issuing the loads
  // of the basis early, and the failing case may take as long as it likes.
  double rmax[4];  // per row of the upper triangle: four short chains instead of one of ten
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    rmax[i] = 0.0;
#pragma unroll
    for (int j = i; j < 4; j++) {
      const double a = fabs(Q[i][j]);
      finite = finite && (a <= 1.7976931348623157e308);  // false for NaN
      rmax[i] = a > rmax[i] ? a : rmax[i];
    }
  }
  const double m01 = rmax[0] > rmax[1] ? rmax[0] : rmax[1], m23 = rmax[2] > rmax[3] ? rmax[2] : rmax[3];
  const double qmax = finite ? (m01 > m23 ? m01 : m23) : 0.0;
  int e;  // 0 for qmax = 0 (coincident points, or a Q that fails anyway)
  (void)frexp(qmax, &e);
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) Q[i][j] = ldexp(Q[i][j], -e);
  bool warm = Vst != nullptr;
  if (warm) {
    bool ortho = true;  // | V^T V - I |_max <= 1e-9, tested per entry: fmax would drop a NaN
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = i; j < 4; j++) {
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) d += V[k][i] * V[k][j];
        ortho = ortho && (fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-9);  // false for NaN
      }
    warm = ortho;
  }
  if (warm) {
    double QV[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) d += Q[i][k] * V[k][j];
        QV[i][j] = d;
      }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = i; j < 4; j++) {
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) d += V[k][i] * QV[k][j];
        Q[i][j] = d;
        Q[j][i] = d;
      }
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
  }
  jacobi4(Q, V);
  if (Vst) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) Vst[4 * i + j] = V[i][j];
  }
  // eigenvector of the largest eigenvalue, picked without dynamic indexing (first maximum wins)
  double ev = Q[0][0];
  double q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
  for (int i = 1; i < 4; i++)
    if (Q[i][i] > ev) {
      ev = Q[i][i];
#pragma unroll
      for (int k = 0; k < 4; k++) q[k] = V[k][i];
    }
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (!finite || !(nrm > 0.0) || !(nrm <= 1.7976931348623157e308)) return false;
  for (int i = 0; i < 4; i++) q[i] /= nrm;
  // CalculateRotation, BaseClass/ICP.cs:274-285
  R1[0] = q[0] * q[0] + q[1] * q[1] - q[2] * q[2] - q[3] * q[3];
  R1[1] = 2.0 * (q[1] * q[2] - q[0] * q[3]);
  R1[2] = 2.0 * (q[1] * q[3] + q[0] * q[2]);
  R1[3] = 2.0 * (q[1] * q[2] + q[0] * q[3]);
  R1[4] = q[0] * q[0] - q[1] * q[1] + q[2] * q[2] - q[3] * q[3];
  R1[5] = 2.0 * (q[2] * q[3] - q[0] * q[1]);
  R1[6] = 2.0 * (q[1] * q[3] - q[0] * q[2]);
  R1[7] = 2.0 * (q[2] * q[3] + q[0] * q[1]);
  R1[8] = q[0] * q[0] - q[1] * q[1] - q[2] * q[2] + q[3] * q[3];
  for (int i = 0; i < 3; i++)
    T1[i] = muY[i] - (R1[3 * i] * muP[0] + R1[3 * i + 1] * muP[1] + R1[3 * i + 2] * muP[2]);
  return true;
}

// The similarity step (vcp.h, "similarity ICP"): horn() on s[0..15] unchanged, then Horn's symmetric scale from the two
// further columns, k = sqrt(vY / vP) with v = sum |x|^2 / N - |mu|^2, which does not depend on the rotation.  c is the
// product of the factors applied so far; the new product c k is held in [ratio_min, ratio_max] by shortening this
// round's factor.  Returns 0 (horn failed: nothing written), 1, or 2 (scale not determined: the rigid step, c stays).
// Every operation is one binary64 rounding; where k_used is 1.0, R1s and T1 are horn()'s bit for bit (1.0 * x = x and
// T1 is horn's expression).
__host__ __device__ inline int horn_sim(const double s[18], long long n, double c, double ratio_min, double ratio_max,
                                        double R1s[9], double T1[3], double* Vst, double* k_used, double* c_new) {
  double R1[9], T1r[3];
  if (!horn(s, n, R1, T1r, Vst)) return 0;
  const double N = (double)n;
  const double muP0 = s[0] / N, muP1 = s[1] / N, muP2 = s[2] / N;  // horn's means: the same divisions
  const double muY0 = s[3] / N, muY1 = s[4] / N, muY2 = s[5] / N;
  const double vP = s[16] / N - ((muP0 * muP0 + muP1 * muP1) + muP2 * muP2);
  const double vY = s[17] / N - ((muY0 * muY0 + muY1 * muY1) + muY2 * muY2);
  const double big = 1.7976931348623157e308;
  const bool det = vP > 0.0 && vP <= big && vY > 0.0 && vY <= big;  // false for NaN
  double ku = 1.0, cn = c;
  if (det) {
    const double k = sqrt(vY / vP), t = c * k;
    if (t < ratio_min) {
      cn = ratio_min;
      ku = ratio_min / c;
    } else if (t > ratio_max) {
      cn = ratio_max;
      ku = ratio_max / c;
    } else {
      cn = t;
      ku = k;
    }
  }
#pragma unroll
  for (int j = 0; j < 9; j++) R1s[j] = ku * R1[j];
  const double muY[3] = {muY0, muY1, muY2};
#pragma unroll
  for (int i = 0; i < 3; i++) T1[i] = muY[i] - (R1s[3 * i] * muP0 + R1s[3 * i + 1] * muP1 + R1s[3 * i + 2] * muP2);
  *k_used = ku;
  *c_new = cn;
  return det ? 1 : 2;
}

// The anisotropic step (vcp.h, "anisotropic ICP"): s[0..17] are sums over the RAW landmarks d (s[16] = sum d0^2,
// s[17] = sum d1^2), and the pose sought is y = R diag(s0, s1, 1) d + t.  One half-step each of a block-coordinate
// descent: per axis a = 0, 1 the least-squares scale for the current rotation R (the problem separates per axis: the
// scale matrix is diagonal), held in [lo_a, hi_a]; then horn() on the sums with rows 0 and 1 of the d-side scaled.  An
// axis whose scale the sums do not determine keeps sc[a]; bit a of *determined says which did.  Returns false where
// horn() fails (nothing but the basis written).  An[9] = Rn diag(sn0, sn1, 1): what the pass applies.  Every operation
// is one binary64 rounding.
__host__ __device__ inline bool horn_aniso(const double (&s)[18], long long n, double* Vst, const double R[9],
                                           const double sc[2], const double lo[2], const double hi[2], double Rn[9],
                                           double Tn[3], double sn[2], double An[9], int* determined) {
  const double N = (double)n;
  const double muY[3] = {s[3] / N, s[4] / N, s[5] / N};
  const double big = 1.7976931348623157e308;
  double sa[2];
  int det = 0;
#pragma unroll
  for (int a = 0; a < 2; a++) {
    const double muD = s[a] / N;
    const double C0 = s[6 + 3 * a] / N - muD * muY[0];
    const double C1 = s[6 + 3 * a + 1] / N - muD * muY[1];
    const double C2 = s[6 + 3 * a + 2] / N - muD * muY[2];
    const double D = s[16 + a] / N - muD * muD;
    const double g = (R[a] * C0 + R[3 + a] * C1) + R[6 + a] * C2;
    const bool ok = D > 0.0 && D <= big && g > 0.0 && g <= big;  // false for NaN
    double v = sc[a];
    if (ok) {
      v = g / D;
      v = v < lo[a] ? lo[a] : v > hi[a] ? hi[a] : v;
      det |= 1 << a;
    }
    sa[a] = v;
  }
  double S[16];
#pragma unroll
  for (int k = 0; k < 16; k++) S[k] = s[k];
#pragma unroll
  for (int a = 0; a < 2; a++) {
    S[a] = sa[a] * s[a];
#pragma unroll
    for (int b = 0; b < 3; b++) S[6 + 3 * a + b] = sa[a] * s[6 + 3 * a + b];
  }
  double R1[9], T1[3];
  if (!horn(S, n, R1, T1, Vst)) return false;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    Rn[3 * i] = R1[3 * i];
    Rn[3 * i + 1] = R1[3 * i + 1];
    Rn[3 * i + 2] = R1[3 * i + 2];
    An[3 * i] = R1[3 * i] * sa[0];
    An[3 * i + 1] = R1[3 * i + 1] * sa[1];
    An[3 * i + 2] = R1[3 * i + 2];
    Tn[i] = T1[i];
  }
  sn[0] = sa[0];
  sn[1] = sa[1];
  *determined = det;
  return true;
}

}  // namespace
