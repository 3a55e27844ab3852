"""Trimmed ICP (include/vcp.h, "trimmed ICP"): what the tests of vcp_icp_sums_trimmed / vcp_icp_trimmed share.  No GPU
here.  It builds on icp_gated_ref (the scene, the brute NN, Kabsch, the conditions, the composition) and icp_sums_ref
(the terms and the replay of the reduction tree):

  * keys / trim_mask: the header's key [K(dd) | index] and the m smallest of them, by a lexsort;
  * keep_count: the header's m for a share;
  * ref_trimmed_icp: a plain numpy binary64 trimmed ICP -- the REFERENCE of the behaviour conditions;
  * trimmed_terms / trimmed_sums: icp_sums_ref's terms with the dropped rows zeroed, through its replay of the tree;
  * replay_run: a whole trimmed run restated round by round from one-pass calls, the host Horn step and the composition.
"""
import math

import numpy as np

import icp_gated_ref as G
import icp_sums_ref as R

SELECT_WG_MAX = 4096   # VCP_ICPT_SELECT_WG_MAX (include/vcp.h): landmarks up to which one workgroup runs the select
NAN_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def keys(dd):
    """K(dd) [n] uint64: the bit pattern of a non-NaN dd (>= +0: the unsigned order is the numeric one), all ones for
    NaN."""
    dd = np.ascontiguousarray(dd, np.float64)
    k = dd.view(np.uint64).copy()
    k[np.isnan(dd)] = NAN_KEY
    return k


def trim_mask(dd, m):
    """(keep [n] bool, thr): the m entries with the smallest keys (K(dd), index) kept; thr = the dd of the kept entry
    with the largest key."""
    dd = np.ascontiguousarray(dd, np.float64)
    n = len(dd)
    if not 1 <= m <= n:
        raise ValueError("m outside [1, n]")
    order = np.lexsort((np.arange(n), keys(dd)))      # last key first: K, then the index
    keep = np.zeros(n, bool)
    keep[order[:m]] = True
    return keep, float(dd[order[m - 1]])


def keep_count(f, L):
    """The header's m = min(L, (int64_t)ceil(f * (double)L)): one multiplication."""
    return min(int(L), int(math.ceil(float(f) * float(L))))


def ref_trimmed_icp(src, tgt, R0, T0, keep, rounds, min_pairs=G.MIN_PAIRS):
    """Trimmed ICP as vcp.h defines it, in numpy: dict(R, T, kept, starved, mean_dist, trim_dist) after `rounds`
    rounds.  keep: the schedule of shares."""
    Rm, T = np.array(R0, np.float64), np.array(T0, np.float64)
    keep = np.atleast_1d(np.asarray(keep, np.float64))
    L = len(src)
    kept, starved, md, td = 0, 0, math.inf, math.nan
    for r in range(1, rounds + 1):
        m = keep_count(keep[min(r, len(keep)) - 1], L)
        p = src @ Rm.T + T
        nn, dd = G.brute_nn(tgt, p)
        mask, thr = trim_mask(dd, m)
        kept = int(mask.sum())
        md = math.sqrt(dd[mask].sum() / kept)
        td = math.sqrt(thr)
        if kept < min_pairs:
            starved += 1
            continue
        R1, T1 = G._kabsch(p[mask], tgt[nn[mask]])
        Rm, T = R1 @ Rm, R1 @ T + T1
    return dict(R=Rm, T=T, kept=kept, starved=starved, mean_dist=md, trim_dist=td)


# ---- one pass through the replayed tree ------------------------------------------------------------------------------
def trimmed_terms(model, data, Rm, T, nn, m):
    """(terms [nd,16] with the dropped rows +0.0, keep [nd] bool, thr): icp_sums_ref.terms and the trim rule on its SSE
    column, which is dd."""
    t = R.terms(model, data, Rm, T, nn)
    keep, thr = trim_mask(t[:, 15], m)
    t[~keep] = 0.0
    return t, keep, thr


def trimmed_sums(model, data, Rm, T, nn, m):
    """What vcp_icp_sums_trimmed must return: (sums [16], keep [nd] uint8, thr)."""
    model = np.ascontiguousarray(model, np.float64).reshape(-1, 3)
    data = np.ascontiguousarray(data, np.float64).reshape(-1, 3)
    t, keep, thr = trimmed_terms(model, data, Rm, T, nn, m)
    pl = R.plan(len(model), len(data), np.isfinite(model).all())
    return R.replay(t, len(data), pl), keep.astype(np.uint8), thr


def same_float(a, b):
    """Equal as binary64 values, NaN equal to NaN."""
    return a == b or (math.isnan(a) and math.isnan(b))


# ---- whole runs, restated from one-pass calls ------------------------------------------------------------------------
def replay_run(ctx, N, tgt, lm, R0, T0, keep, rounds, min_pairs=G.MIN_PAIRS):
    """[per round: dict(M [4,4], mean_dist, kept, starved, trim_dist)]: each round is icp_sums_trimmed at that round's m
    from the state so far, then -- unless starved -- the host Horn step on (sums, m) with the carried basis and the
    composition."""
    Rm = [float(x) for x in np.asarray(R0).reshape(9)]
    T = [float(x) for x in np.asarray(T0).reshape(3)]
    keep = np.atleast_1d(np.asarray(keep, np.float64))
    V = np.zeros(16)
    starved = 0
    out = []
    for r in range(1, rounds + 1):
        m = keep_count(keep[min(r, len(keep)) - 1], len(lm))
        S, thr, _, _ = ctx.icp_sums_trimmed(tgt, lm, m, np.array(Rm).reshape(3, 3), np.array(T), want_nn=False,
                                            want_keep=False)
        if m < min_pairs:
            starved += 1
        else:
            R1, T1, V = G._horn(N, S, m, V)
            Rm, T = G._compose(R1, T1, Rm, T)
        M = np.eye(4)
        M[:3, :3] = np.array(Rm).reshape(3, 3)
        M[:3, 3] = T
        out.append(dict(M=M, mean_dist=math.sqrt(float(S[15]) / m), kept=m, starved=starved,
                        trim_dist=math.sqrt(thr)))
    return out
