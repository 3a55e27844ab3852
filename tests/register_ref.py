"""vcp_register_pairs's definition (include/vcp.h, "congruent-pair global registration") restated in plain numpy, and what
its tests share.  No GPU here.

  * register(): every length of an ordered target pair at once, the header's test against every base, then every
    hypothesis scored by a brute-force existence test over all targets.  numpy rounds every binary64 operation on its
    own, sqrt and / correctly, so the device is compared with this for EQUALITY: score, pick, n_hyp, inliers, best and
    the bits of M_all and M_best;
  * overlap_scene(): the partial-overlap scene of the behaviour claim (a scan that sees a window of the truth field);
  * centroid_start_best(): the 36-start centroid-start loops that scene defeats, by icp_gated_ref.ref_icp.
"""
import functools
import math

import numpy as np

OK, ERR_ARG, ERR_EMPTY, ERR_INDEX, ERR_TOO_LARGE, ERR_UNSUPPORTED = 0, -1, -2, -4, -5, -8
MAX_BASES, MAX_TARGETS = 4096, 65536
_CELLS = 4_000_000          # hypotheses x landmarks x targets scored per numpy call


class RefError(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


def landmark_indices(ns, max_landmarks):
    step = ns // max_landmarks if ns > max_landmarks else 1
    return np.arange(ns // step) * step


def transform(M, p):
    """[H, n, 3]: every p [n, 3] under every M [H, 4, 4]: row by row, left to right, all four terms."""
    x, y, z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    out = np.empty((len(M), len(p), 3))
    for r in range(3):
        out[:, :, r] = ((x * M[:, r, 0, None] + y * M[:, r, 1, None]) + z * M[:, r, 2, None]) + M[:, r, 3, None]
    return out


def count_near(M, p, tgt, dist):
    """[H]: how many p have SOME target with sqrt(dx*dx + dy*dy + dz*dz) < dist under each M."""
    out = np.zeros(len(M), np.int64)
    if len(M) == 0:
        return out
    per = max(1, _CELLS // max(1, len(p) * len(tgt)))
    with np.errstate(all="ignore"):
        for a in range(0, len(M), per):
            m = transform(M[a:a + per], p)
            dx = tgt[None, None, :, 0] - m[:, :, None, 0]
            dy = tgt[None, None, :, 1] - m[:, :, None, 1]
            dz = tgt[None, None, :, 2] - m[:, :, None, 2]
            d = np.sqrt((dx * dx + dy * dy) + dz * dz)
            out[a:a + per] = (d < dist).any(axis=2).sum(axis=1)
    return out


def poses(src, tgt, a, b, f, i, j):
    """(M [H,4,4], ok [H]) of the hypotheses (base (a, b), flip f, targets (i, j) [H]): the header's formulas in their
    operand order.  ok False: skipped (nrm)."""
    i, j = np.asarray(i), np.asarray(j)
    H = len(i)
    sgn = -1.0 if f else 1.0
    ax, ay, az = src[a, 0], sgn * src[a, 1], src[a, 2]
    bx, by, bz = src[b, 0], sgn * src[b, 1], src[b, 2]
    ux, uy = bx - ax, by - ay
    msx, msy, msz = (ax + bx) * 0.5, (ay + by) * 0.5, (az + bz) * 0.5
    ti, tj = tgt[i], tgt[j]
    with np.errstate(all="ignore"):
        vx, vy = tj[:, 0] - ti[:, 0], tj[:, 1] - ti[:, 1]
        dot, crs = ux * vx + uy * vy, ux * vy - uy * vx
        nrm = np.sqrt(dot * dot + crs * crs)
        ok = (nrm > 0.0) & (nrm < np.inf)
        c, s = dot / nrm, crs / nrm
        mt = (ti + tj) * 0.5
        M = np.zeros((H, 4, 4))
        M[:, 0, 0], M[:, 1, 0] = c, s
        if f:
            M[:, 0, 1], M[:, 1, 1] = s, -c
        else:
            M[:, 0, 1], M[:, 1, 1] = -s, c
        M[:, 2, 2] = M[:, 3, 3] = 1.0
        M[:, 0, 3] = mt[:, 0] - (c * msx - s * msy)
        M[:, 1, 3] = mt[:, 1] - (s * msx + c * msy)
        M[:, 2, 3] = mt[:, 2] - msz
    return M, ok


def candidates(src, tgt, bases, len_tol, rows=512):
    """Per base the ordered target pairs (i [n], j [n]) of its length, ascending in (i, j); empty where Lu is not in
    (0, inf).  Also Lu [B]."""
    B, nt = len(bases), len(tgt)
    with np.errstate(all="ignore"):
        ux = src[bases[:, 1], 0] - src[bases[:, 0], 0]
        uy = src[bases[:, 1], 1] - src[bases[:, 0], 1]
        Lu = np.sqrt(ux * ux + uy * uy)
    live = (Lu > 0.0) & (Lu < np.inf)
    got = [([], []) for _ in range(B)]
    for r0 in range(0, nt, rows):
        with np.errstate(all="ignore"):
            vx = tgt[None, :, 0] - tgt[r0:r0 + rows, None, 0]      # v = t_j - t_i: i down the rows, j along them
            vy = tgt[None, :, 1] - tgt[r0:r0 + rows, None, 1]
            Lv = np.sqrt(vx * vx + vy * vy)
            pair = (Lv > 0.0) & (Lv < np.inf)
            k = np.arange(r0, min(r0 + rows, nt))
            pair[k - r0, k] = False                               # i != j (Lv = 0 there anyway)
            for b in np.flatnonzero(live):
                ii, jj = np.nonzero(pair & (np.abs(Lv - Lu[b]) <= len_tol))
                if len(ii):
                    got[b][0].append(ii + r0)
                    got[b][1].append(jj)
    e = np.zeros(0, np.int64)
    return [(np.concatenate(g[0]) if g[0] else e, np.concatenate(g[1]) if g[1] else e) for g in got], Lu


def check_arguments(ns, nt, bases, len_tol, max_landmarks, inlier_dist):
    B = len(bases)
    if B < 1 or max_landmarks < 1 or not (len_tol >= 0.0) or not (inlier_dist > 0.0):
        raise RefError(ERR_ARG)
    if ns < 2 or nt < 2:
        raise RefError(ERR_EMPTY)
    if B > MAX_BASES or nt > MAX_TARGETS:
        raise RefError(ERR_UNSUPPORTED)
    if ((bases < 0) | (bases >= ns)).any():
        raise RefError(ERR_INDEX)


def register(source, target, bases, len_tol, inlier_dist, mirror=False, max_landmarks=200):
    """dict(best, M [4,4], M_all [B,4,4], score [B], inliers [B], pick [B,3], n_hyp [B]) as the header defines them."""
    src = np.ascontiguousarray(source, np.float64).reshape(-1, 3)
    tgt = np.ascontiguousarray(target, np.float64).reshape(-1, 3)
    bases = np.asarray(bases, np.int64).reshape(-1, 2)
    check_arguments(len(src), len(tgt), bases, len_tol, max_landmarks, inlier_dist)
    B = len(bases)
    lm = src[landmark_indices(len(src), max_landmarks)]
    cand, _ = candidates(src, tgt, bases, len_tol)
    M_all = np.zeros((B, 4, 4))
    score = np.full(B, -1, np.int32)
    inliers = np.zeros(B, np.int32)
    pick = np.tile(np.array([0, -1, -1], np.int32), (B, 1))
    n_hyp = np.zeros(B, np.int64)
    # every hypothesis of every base in one list, base by base and ascending in (i, j) inside a base
    cnt = np.array([len(c[0]) for c in cand], np.int64)
    start = np.concatenate([[0], np.cumsum(cnt)])
    hb = np.repeat(np.arange(B), cnt)
    ii = np.concatenate([c[0] for c in cand]).astype(np.int64)
    jj = np.concatenate([c[1] for c in cand]).astype(np.int64)
    for f in ((0, 1) if mirror else (0,)):                        # ascending (f, i, j): the first maximum wins
        n_hyp += cnt
        M, ok = poses(src, tgt, bases[hb, 0], bases[hb, 1], f, ii, jj)
        sc = np.full(len(hb), -1, np.int64)                       # a skipped hypothesis (nrm) cannot win
        sc[ok] = count_near(M[ok], lm, tgt, inlier_dist)
        for b in np.flatnonzero(cnt):
            seg = sc[start[b]:start[b + 1]]
            w = int(np.argmax(seg))                               # the first of the maxima
            if seg[w] > score[b]:
                k = start[b] + w
                score[b], M_all[b], pick[b] = seg[w], M[k], (f, ii[k], jj[k])
    won = np.flatnonzero(score >= 0)
    inliers[won] = count_near(M_all[won], src, tgt, inlier_dist)
    best = -1
    for b in range(B):
        if score[b] >= 0 and (best < 0 or inliers[b] > inliers[best] or
                              (inliers[b] == inliers[best] and score[b] > score[best])):
            best = b
    return dict(best=best, M=M_all[best].copy() if best >= 0 else np.eye(4), M_all=M_all, score=score, inliers=inliers,
                pick=pick, n_hyp=n_hyp)


def same(got, ref):
    """Asserts that a device result equals the reference's: integers for equality, matrices bit for bit."""
    for k in ("score", "pick", "n_hyp", "inliers"):
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    assert got["best"] == ref["best"], (got["best"], ref["best"])
    for k in ("M_all", "M"):
        a, b = np.ascontiguousarray(got[k], np.float64), np.ascontiguousarray(ref[k], np.float64)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), k


# ---- the partial-overlap scene ------------------------------------------------------------------------------------------
ANGLE, SHIFT = 2.0, (1.5, -0.8, 0.0)      # the planted pose: source -> truths
FIELD, NOISE, KEEP, CLUTTER = 20.0, 0.01, 0.9, 10
LEN_TOL, INLIER = 0.03, 0.1
N_BASES, MIN_LEN, MAX_LEN = 8, 2.0, 5.0
POLISH = (0.3, 0.1, 5, 20)                # gates 0.3 -> 0.1 over 5 rounds, 20 rounds
# (window edge, scene seed, choose_bases seed): fixed after tests/test_register.py showed the conditions hold on them
SCENES = {"half": (10.0, 5, 1), "third": (7.0, 6, 2)}


def rz(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def planted():
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = rz(ANGLE), SHIFT
    return M


def overlap_scene(window, seed, n_truths=400):
    """dict(truths [400,3] uniform in [0,20]^2, z = 0; source: the truths inside [0, window]^2, 90 % kept, noise sigma 0.01,
    plus 10 clutter points in the window, shuffled and moved back by the planted pose; planted = that pose's inlier
    count at 0.1)."""
    rng = np.random.default_rng([seed, n_truths])
    truths = np.zeros((n_truths, 3))
    truths[:, :2] = rng.uniform(0.0, FIELD, (n_truths, 2))
    seen = truths[(truths[:, 0] <= window) & (truths[:, 1] <= window)]
    seen = seen[rng.random(len(seen)) < KEEP].copy()
    seen[:, :2] += rng.normal(0.0, NOISE, (len(seen), 2))
    clutter = np.zeros((CLUTTER, 3))
    clutter[:, :2] = rng.uniform(0.0, window, (CLUTTER, 2))
    x = np.concatenate([seen, clutter])
    x = x[rng.permutation(len(x))]
    source = np.ascontiguousarray((x - np.array(SHIFT)) @ rz(ANGLE))      # Rz source + T = x
    source[:, 2] = 0.0
    n = int(count_near(planted()[None], source, truths, INLIER)[0])
    return dict(truths=np.ascontiguousarray(truths), source=source, planted=n)


@functools.lru_cache(maxsize=None)
def scene_case(name):
    """(scene, bases, reference result) of SCENES[name], computed once per process."""
    from vtkcloudpoint_amd.icp import choose_bases
    window, seed, bseed = SCENES[name]
    sc = overlap_scene(window, seed)
    bases = choose_bases(sc["source"], N_BASES, MIN_LEN, MAX_LEN, bseed)
    return sc, bases, register(sc["source"], sc["truths"], bases, LEN_TOL, INLIER)


def inliers_of(sc, R, T):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, T
    return int(count_near(M[None], sc["source"], sc["truths"], INLIER)[0])


def centroid_start_best(sc, n_angles=36, rounds=60):
    """The most inliers any of the 2 * n_angles centroid-start runs reaches: Rz(h 2 pi / n) from T0 = mean(target) - R0
    mean(source), ungated and gated (1.8 -> 0.3, geometric, over 10 rounds)."""
    import icp_gated_ref as G
    from vtkcloudpoint_amd.icp import gate_schedule
    src, tgt = sc["source"], sc["truths"]
    ms, mt = src.mean(axis=0), tgt.mean(axis=0)
    best = 0
    for gates in (None, gate_schedule(1.8, 0.3, 10)):
        for h in range(n_angles):
            R0 = rz(h * (2.0 * math.pi / n_angles))
            r = G.ref_icp(src, tgt, R0, mt - R0 @ ms, gates, rounds)
            best = max(best, inliers_of(sc, r["R"], r["T"]))
    return best
