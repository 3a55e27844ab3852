"""Unique-correspondence ICP (include/vcp.h, "unique-correspondence ICP"): what the tests of vcp_icp_sums_unique /
vcp_icp_unique share.  No GPU here.  It builds on icp_gated_ref (the scene, the brute NN, the drop rule, Kabsch, the
conditions, the composition), icp_trimmed_ref (the key K(dd)) and icp_sums_ref (the terms and the replay of the tree):

  * unique_mask: the header's winner per target, by a lexsort over (nn, K(dd), index);
  * ref_unique_icp: a plain numpy binary64 loop -- the REFERENCE of the behaviour conditions;
  * unique_terms / unique_sums: icp_sums_ref's terms with the dropped rows zeroed, through its replay of the tree;
  * replay_run: a whole run restated round by round from one-pass calls, the host Horn step and the composition;
  * ghost_scene: icp_gated_ref.scene with a second centroid beside 40 % of the true ones.
"""
import math

import numpy as np

import icp_gated_ref as G
import icp_sums_ref as R
import icp_trimmed_ref as TR

GHOST_SHARE = 0.4               # of the true centroids get a ghost
GHOST_OFFSET = (0.07, 0.0)      # from the truth, in the truth frame: the same side for every ghost
# fixed after tests/test_icp_unique.py showed that its conditions hold on them (per size: the gated scene's own seed,
# then one more)
SEEDS = {40: (1, 11), 300: (2, 12), 600: (3, 13)}


def unique_mask(nn, dd):
    """win [n] bool: per target j the landmark with the smallest key (K(dd), index) among those with nn == j."""
    nn = np.asarray(nn, np.int64)
    n = len(nn)
    order = np.lexsort((np.arange(n), TR.keys(dd), nn))      # last key first: the target, then K, then the index
    first = np.ones(n, bool)
    first[1:] = nn[order][1:] != nn[order][:-1]
    win = np.zeros(n, bool)
    win[order[first]] = True
    return win


def keep_codes(nn, dd, gate):
    """[n] uint8 as vcp_icp_sums_unique's keep: 2 not the winner, 0 winner dropped by the gate, 1 kept."""
    win = unique_mask(nn, dd)
    kept = win & G.kept_mask(np.asarray(dd, np.float64), gate)
    return np.where(win, kept.astype(np.uint8), np.uint8(2)).astype(np.uint8)


def ref_unique_icp(src, tgt, R0, T0, gates, rounds, min_pairs=G.MIN_PAIRS):
    """Unique-correspondence ICP as vcp.h defines it, in numpy: dict(R, T, kept, lost, starved, mean_dist) after
    `rounds` rounds."""
    Rm, T = np.array(R0, np.float64), np.array(T0, np.float64)
    kept, lost, starved, md = 0, 0, 0, math.inf
    for r in range(1, rounds + 1):
        g = float(gates[min(r, len(gates)) - 1])
        p = src @ Rm.T + T
        nn, dd = G.brute_nn(tgt, p)
        code = keep_codes(nn, dd, g)
        keep = code == 1
        kept, lost = int(keep.sum()), int((code == 2).sum())
        md = math.sqrt(dd[keep].sum() / kept) if kept else math.inf
        if kept < min_pairs:
            starved += 1
            continue
        R1, T1 = G._kabsch(p[keep], tgt[nn[keep]])
        Rm, T = R1 @ Rm, R1 @ T + T1
    return dict(R=Rm, T=T, kept=kept, lost=lost, starved=starved, mean_dist=md)


# ---- one pass through the replayed tree ------------------------------------------------------------------------------
def unique_terms(model, data, Rm, T, nn, gate):
    """(terms [nd,16] with the dropped rows +0.0, code [nd] uint8): icp_sums_ref.terms and the rule on its SSE column,
    which is dd."""
    t = R.terms(model, data, Rm, T, nn)
    code = keep_codes(nn, t[:, 15], gate)
    t[code != 1] = 0.0
    return t, code


def unique_sums(model, data, Rm, T, nn, gate):
    """What vcp_icp_sums_unique must return: (sums [16], kept, lost, keep [nd] uint8)."""
    model = np.ascontiguousarray(model, np.float64).reshape(-1, 3)
    data = np.ascontiguousarray(data, np.float64).reshape(-1, 3)
    t, code = unique_terms(model, data, Rm, T, nn, gate)
    pl = R.plan(len(model), len(data), np.isfinite(model).all())
    return R.replay(t, len(data), pl), int((code == 1).sum()), int((code == 2).sum()), code


# ---- whole runs, restated from one-pass calls ------------------------------------------------------------------------
def replay_run(ctx, N, tgt, lm, R0, T0, gates, rounds, min_pairs=G.MIN_PAIRS):
    """[per round: dict(M [4,4], mean_dist, kept, lost, starved, nn, keep)]: each round is icp_sums_unique at that
    round's gate from the state so far, then -- unless starved -- the host Horn step on (sums, kept) with the carried
    basis and the composition."""
    Rm = [float(x) for x in np.asarray(R0).reshape(9)]
    T = [float(x) for x in np.asarray(T0).reshape(3)]
    V = np.zeros(16)
    starved = 0
    out = []
    for r in range(1, rounds + 1):
        g = float(gates[min(r, len(gates)) - 1])
        S, kept, lost, nn, keep = ctx.icp_sums_unique(tgt, lm, g, np.array(Rm).reshape(3, 3), np.array(T))
        if kept < min_pairs:
            starved += 1
        else:
            R1, T1, V = G._horn(N, S, kept, V)
            Rm, T = G._compose(R1, T1, Rm, T)
        M = np.eye(4)
        M[:3, :3] = np.array(Rm).reshape(3, 3)
        M[:3, 3] = T
        out.append(dict(M=M, mean_dist=math.sqrt(float(S[15]) / kept) if kept else math.inf, kept=kept, lost=lost,
                        starved=starved, nn=nn, keep=keep))
    return out


# ---- the scene -------------------------------------------------------------------------------------------------------
def ghost_scene(nt, ntrue, nclutter, seed):
    """icp_gated_ref.scene(nt, ntrue, nclutter, seed) plus a ghost beside GHOST_SHARE of the true centroids: each at its
    truth + GHOST_OFFSET in the truth frame with the scene's noise on top, shuffled in with the other centroids, moved
    back by the true pose and marked not true.  Further keys: n_ghost, is_ghost [n], bias = the pull the ghosts put on a
    fit that takes every pair, |GHOST_OFFSET| g / (n + g) with g ghosts among n true centroids."""
    sc = G.scene(nt, ntrue, nclutter, seed)
    rng = np.random.default_rng([seed, nt, 40])
    true_idx = np.flatnonzero(sc["is_true"])
    g = int(round(GHOST_SHARE * ntrue))
    chosen = rng.permutation(true_idx)[:g]
    x = sc["truths"][sc["truth_of"][chosen]].copy()
    x[:, 0] += GHOST_OFFSET[0]
    x[:, 1] += GHOST_OFFSET[1]
    x[:, :2] += rng.normal(0.0, G.NOISE, (g, 2))
    ghosts = np.ascontiguousarray((x - sc["T_true"]) @ sc["R_true"])
    ghosts[:, 2] = 0.0
    n0 = len(sc["centers"])
    perm = rng.permutation(n0 + g)
    out = dict(sc)
    out["centers"] = np.ascontiguousarray(np.concatenate([sc["centers"], ghosts])[perm])
    out["truth_of"] = np.concatenate([sc["truth_of"], np.full(g, -1)])[perm]
    out["is_true"] = out["truth_of"] >= 0
    out["is_ghost"] = (np.arange(n0 + g) >= n0)[perm]
    out["n_ghost"] = g
    out["bias"] = math.hypot(*GHOST_OFFSET) * g / (ntrue + g)
    return out
