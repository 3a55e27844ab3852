"""csrc/wave.hpp on the MI355X: vcp_selftest_wave_dev runs every helper in one workgroup of tb threads on words and flags
of the test's, and each row of its output is held to numpy, sums modulo 2^32 (include/vcp.h lists the rows).  Sizes: one
thread, one short of a wave, a wave, one more, one short of the workgroup and all of it, for workgroups of 1, 4, 8 and 16
waves; flags all clear, all set, only lane 0 or only lane 63 of every wave, and random; words random and all 0xFFFFFFFF
(every sum wraps).  The signed 64-bit all-reduce (sum, maximum, minimum) runs on (v - 2^31) * 2^20, values of both signs
whose sums leave 32 bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = 24
M32 = (1 << 32) - 1
NOSLOT = 0xFFFFFFFF
START = 0xFFFFFF00  # the append counter's start: the slots of a large workgroup wrap


def reference(v, p, tb):
    """Every row but the append's (14), as uint64 arrays of tb entries."""
    v64 = v.astype(np.uint64)
    cs = np.cumsum(v64)
    pc = np.cumsum(p.astype(np.uint64))
    P = int(pc[-1])
    waves = v64.reshape(-1, 64)
    per_wave = lambda a: np.repeat(a.astype(np.uint64), 64)
    only0 = lambda x: np.array([x] + [NOSLOT] * (tb - 1), np.uint64)
    prev = np.roll(v64, 1)
    prev[0::64] = v64[0::64]
    r = {
        0: (cs - v64) & M32, 1: (cs - v64) & M32, 2: np.full(tb, int(cs[-1]) & M32, np.uint64),
        3: per_wave(waves.sum(1) & M32), 4: per_wave(waves.min(1)), 5: per_wave(waves.max(1)),
        6: per_wave(np.bitwise_or.reduce(waves, 1)), 7: per_wave(p.reshape(-1, 64).sum(1)),
        8: only0(P), 9: only0(P), 10: only0(int((v & 1).sum())),
        11: np.where(p, pc - p, 0), 12: pc - p, 13: np.full(tb, P, np.uint64),
        15: np.maximum.accumulate(waves, 1).reshape(-1),
        16: np.cumsum(v64.reshape(-1, 32), 1).reshape(-1) & M32, 17: prev,
    }
    # rows 18..23: s = (v - 2^31) * 2^20 in signed 64 bits (Python integers here); sum modulo 2^64, maximum, minimum
    s = [[(int(x) - (1 << 31)) << 20 for x in wave] for wave in waves.tolist()]
    for row, f in ((18, sum), (20, max), (22, min)):
        u = [f(wave) & ((1 << 64) - 1) for wave in s]
        r[row] = per_wave(np.array([x & M32 for x in u], np.uint64))
        r[row + 1] = per_wave(np.array([x >> 32 for x in u], np.uint64))
    return r, P


@pytest.mark.parametrize("tb", [64, 256, 512, 1024])
def test_wave_helpers(vcp_ctx, tb):
    rng = np.random.default_rng(tb)
    d_words = torch.zeros(tb, dtype=torch.int32, device="cuda")
    d_flags = torch.zeros(tb, dtype=torch.uint8, device="cuda")
    d_counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(ROWS * tb, dtype=torch.int32, device="cuda")
    lanes = np.arange(tb) & 63
    for n in sorted({1, 63, 64, 65, tb - 1, tb} & set(range(1, tb + 1))):
        flag_sets = {"clear": np.zeros(tb, bool), "set": np.ones(tb, bool), "lane0": lanes == 0, "lane63": lanes == 63,
                     "random": rng.integers(0, 2, tb).astype(bool)}
        word_sets = {"random": rng.integers(0, 1 << 32, tb, dtype=np.uint64).astype(np.uint32),
                     "ones": np.full(tb, M32, np.uint32)}
        for fname, f in flag_sets.items():
            for wname, w in word_sets.items():
                what = "tb %d n %d flags %s words %s" % (tb, n, fname, wname)
                v, p = w.copy(), f.copy()
                v[n:] = 0
                p[n:] = False
                # the device reads n entries; what lies behind them must not matter
                d_words.copy_(torch.from_numpy(w.view(np.int32)))
                d_flags.copy_(torch.from_numpy(f.astype(np.uint8) * 3))
                d_counter.fill_(START - (1 << 32))
                d_out.fill_(-1)
                torch.cuda.synchronize()
                vcp_ctx.selftest_wave_dev(d_words.data_ptr(), d_flags.data_ptr(), n, tb, d_counter.data_ptr(),
                                          d_out.data_ptr())
                out = d_out.cpu().numpy().view(np.uint32).reshape(ROWS, tb).astype(np.uint64)
                ref, P = reference(v, p, tb)
                for r, want in ref.items():
                    assert np.array_equal(out[r], want), "%s: row %d" % (what, r)
                # the append: the slots are a permutation of [start, start + P) modulo 2^32, in lane order inside a wave
                assert int(d_counter.cpu().numpy().view(np.uint32)[0]) == (START + P) & M32, what
                assert np.all(out[14][~p] == NOSLOT), what
                rel = (out[14].astype(np.int64) - START) & M32  # slots relative to the start
                assert sorted(rel[p].tolist()) == list(range(P)), what
                for wv in range(tb // 64):
                    mine = rel[wv * 64:(wv + 1) * 64][p[wv * 64:(wv + 1) * 64]]
                    assert np.all(np.diff(mine) == 1), "%s: wave %d" % (what, wv)

