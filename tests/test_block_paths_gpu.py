"""Every path of the block pipeline (csrc/blockpart.hip, csrc/blocks.hip) against the CPU oracle, bit for bit, with proof
from the library's own trace (VCP_TRACE) that the path meant is the path that ran: the case table of
tests/block_path_cases.py under the default switches and under each of the pipeline's own developer switches.

The switches are read once per process, so every setting is a fresh child (tests/_block_paths_worker.py) that runs the whole
table, every case as the one public call and once more stage by stage; VCP_TRACE=1 and the switch are the only VCP_*
variables it sees.  The child compares every output with the oracle (and, for the position cases, with the numpy restatement
of the partition).  The parent holds what the library traced between a case's markers to block_path_cases.model(inp) --
every field of the `blocks plan`, `blocks build`, `blocks cluster`, `blocks partition`, `blocks order` and `blocks noise`
lines -- and the launches to block_path_cases.sites: the sites that must appear and those that must not.  It checks that
each switch took effect somewhere.  The children run one after another; if one ends by signal, abort or time limit, no
further child is started and the remaining tests fail at once, naming it.

Wall time of a child on the MI355X, start-up and the oracle's side included (limit: 120 s each):
default 2.8 s, brute_max_0 2.8 s, blocks_order_sort 2.8 s, noise_all 2.8 s."""
import os
import subprocess
import sys
import time

import pytest

import block_path_cases as T
from engine_path_cases import parse_trace_line

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_block_paths_worker.py")
CHILD_TIMEOUT = 120  # seconds; a third of it is the most a child may need before its table is split

SETTINGS = {
    "default": {},
    "brute_max_0": {"VCP_BRUTE_MAX": "0"},
    "blocks_order_sort": {"VCP_BLOCKS_ORDER_SORT": "1"},
    "noise_all": {"VCP_NOISE_ALL": "1"},
}
MODEL_SWITCH = {"brute_max_0": dict(brute_thr=0), "blocks_order_sort": dict(order_sort=True)}

_runs, _fatal, _models, walls = {}, [], {}, {}


class CaseRun:
    def __init__(self):
        self.status, self.launches, self.lines = None, [], []

    def words(self, word):
        return [d for what, d in self.lines if what == "blocks" and d.get("_words") == [word]]


def parse(stderr):
    run, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith("@@ begin "):
            cur = run[line[9:].strip()] = CaseRun()
        elif line.startswith("@@ end "):
            name, _, rest = line[7:].partition(" ")
            run[name].status = rest.strip()
            cur = None
        elif line.startswith("vcp-trace ") and cur is not None:
            what, payload = parse_trace_line(line)
            if what == "launch":
                cur.launches.append(payload)
            else:
                cur.lines.append((what, payload))
    return run


def get_run(setting):
    """The child of one setting, started once; after a child that ended by signal, abort or time limit, nothing starts."""
    if setting in _runs:
        return _runs[setting]
    if _fatal:
        pytest.fail("not started: " + _fatal[0])
    env = {k: v for k, v in os.environ.items() if not k.startswith("VCP_")}
    env["VCP_TRACE"] = "1"
    env.update(SETTINGS[setting])
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, WORKER], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        tail = (e.stderr or b"")[-1500:]
        _fatal.append("the child of setting %s ran into its time limit of %d s:\n%s" % (
            setting, CHILD_TIMEOUT, tail.decode(errors="replace") if isinstance(tail, bytes) else tail))
        pytest.fail(_fatal[0])
    walls[setting] = time.time() - t0
    print("child %s: %.1f s" % (setting, walls[setting]))
    if p.returncode not in (0, 1):
        _fatal.append("the child of setting %s ended with status %d:\n%s\n%s" % (setting, p.returncode, p.stdout[-1000:],
                                                                                 p.stderr[-3000:]))
        pytest.fail(_fatal[0])
    run = parse(p.stderr)
    names = [c.name + form for c in T.CASES for form in ("", "/staged")]
    missing = [nm for nm in names if nm not in run or run[nm].status is None]
    assert not missing, "cases without a result: %r\n%s" % (missing[:5], p.stderr[-2000:])
    _runs[setting] = run
    return run


def model_of(case, setting):
    key = (case.name, setting if setting in MODEL_SWITCH else "default")
    if key not in _models:
        inp = case.build()
        _models[key] = (inp, T.model(inp, **MODEL_SWITCH.get(setting, {})))
    return _models[key]


def _fields(got, want, what):
    return [] if got == want else ["`blocks %s` shows %r, the model says %r" % (
        what, {k: got.get(k) for k in want if got.get(k) != want[k]}, {k: want[k] for k in want if got.get(k) != want[k]})]


def check_case(case, cr, setting, staged):
    """-> list of complaints about one case under one setting, as one call or staged"""
    bad = []
    if cr.status != "ok":
        bad.append("differs from the oracle: " + cr.status)
    inp, M = model_of(case, setting)
    must = T.sites(M, staged)
    seen = set(cr.launches) & T.SITES
    if must - seen:
        bad.append("launch sites missing from the trace: %r" % sorted(must - seen))
    if seen - must:
        bad.append("launch sites that must not run: %r" % sorted(seen - must))
    plans, builds, clusters = cr.words("plan"), cr.words("build"), cr.words("cluster")
    if M["error"]:
        if cr.lines:
            bad.append("a call that fails in the selection traced %r" % cr.lines)
        return bad
    if len(plans) != 1 or len(builds) != 1:
        return bad + ["%d `blocks plan` and %d `blocks build` lines for one call" % (len(plans), len(builds))]
    strip = lambda d: {k: v for k, v in d.items() if k != "_words"}  # noqa: E731
    bad += _fields(strip(plans[0]), M["plan"], "plan") + _fields(strip(builds[0]), M["build"], "build")
    want = M["cluster"]
    if not staged:
        if len(clusters) != 1:
            return bad + ["%d `blocks cluster` lines for one call" % len(clusters)]
        bad += _fields(strip(clusters[0]), dict(want, lo=0, hi=M["plan"]["nblocks"]), "cluster")
    else:  # the shares adjoin and cover every block; an empty share traces nothing
        spans = sorted((d["lo"], d["hi"]) for d in clusters)
        if not spans or spans[0][0] != 0 or spans[-1][1] != M["plan"]["nblocks"] or \
                any(a[1] != b[0] for a, b in zip(spans, spans[1:])):
            bad.append("the shares' `blocks cluster` lines cover %r" % spans)
        got = dict(pts_small=sum(d["pts_small"] for d in clusters), any_mid=int(any(d["any_mid"] for d in clusters)),
                   pts_big=sum(d["pts_big"] for d in clusters) if want["pts_small"] or want["pts_big"] != 1 else 1)
        bad += _fields(got, want, "cluster (summed over the shares)")
    thr = [d["brute_thr"] for d in cr.words("partition")]
    if thr != [0 if setting == "brute_max_0" else T.VCP_BRUTE_MAX]:
        bad.append("`blocks partition` shows brute_thr %r" % thr)
    orders = [strip(d) for d in cr.words("order")]
    if orders != T.order_lines(M, staged):
        bad.append("`blocks order` lines %r, the model says %r" % (orders, T.order_lines(M, staged)))
    noise = [d["all_active"] for d in cr.words("noise")]
    all_active = int("key_xy" in inp or setting == "noise_all")
    if not noise or set(noise) != {all_active} or len(noise) != len(orders) - (len(orders) // 2 if staged else 0):
        bad.append("`blocks noise` lines %r for all_active = %d" % (noise, all_active))
    return bad


def check_table(setting):
    run = get_run(setting)
    bad = []
    for case in T.CASES:
        for form in ("", "/staged"):
            bad += ["%s%s: %s" % (case.name, form, b) for b in check_case(case, run[case.name + form], setting, bool(form))]
    assert not bad, "%d complaints under %s:\n%s" % (len(bad), setting, "\n".join(bad[:40]))
    assert walls[setting] < CHILD_TIMEOUT / 3, "the child took %.1f s: split this setting's table" % walls[setting]
    return run


def _all(run, word, key):
    return [d[key] for cr in run.values() for d in cr.words(word)]


def test_default():
    run = check_table("default")
    # what the switch tests below compare against, and every row of the table on both of its sides
    assert set(_all(run, "partition", "brute_thr")) == {T.VCP_BRUTE_MAX}
    assert set(_all(run, "noise", "all_active")) == {0, 1}  # (1: the keyed case)
    orders = [d for cr in run.values() for d in cr.words("order")]
    assert any(d["by_sort"] == 0 for d in orders) and any(d.get("retry") == 1 for d in orders)
    assert all(d["by_sort"] == 1 for d in orders if d.get("retry"))
    assert {1, 2, 7} <= set(_all(run, "plan", "passes")) and {0, 1, 10} <= set(_all(run, "plan", "fsh"))
    assert set(_all(run, "plan", "keyed")) == {0, 1} and set(_all(run, "cluster", "any_mid")) == {0, 1}
    assert any(v > 16384 for v in _all(run, "plan", "NS")) and any(v > 1 for v in _all(run, "build", "nslice"))
    for case in T.CASES:  # the claim each case exists for, on the traced values themselves
        if T.model(case.build())["error"]:
            continue
        cr = run[case.name]
        got = {"plan": cr.words("plan")[0], "build": cr.words("build")[0], "cluster": cr.words("cluster")[0],
               "retry": any(d.get("retry") for d in cr.words("order"))}
        for key, want in case.want.items():
            if key.split(".")[0] in got:
                v = T.lookup(got, key)
                assert want(v) if callable(want) else v == want, "%s: the trace shows %s = %r" % (case.name, key, v)


def test_brute_max_0():
    run = check_table("brute_max_0")
    assert set(_all(run, "partition", "brute_thr")) == {0}
    assert set(_all(run, "cluster", "pts_small")) == {0}
    launches = {k for cr in run.values() for k in cr.launches}
    assert not launches & {T.BRUTE_SMALL, T.BRUTE_MID, "k_zero_words"}, "the all-pairs kernel ran with VCP_BRUTE_MAX=0"


def test_blocks_order_sort():
    run = check_table("blocks_order_sort")
    orders = [d for cr in run.values() for d in cr.words("order")]
    assert orders and all(d["by_sort"] == 1 and "retry" not in d for d in orders)
    launches = {k for cr in run.values() for k in cr.launches}
    assert not launches & {"k_block_order", "k_block_order_big"} and "k_cluster_sizes" in launches


def test_noise_all():
    run = check_table("noise_all")
    assert set(_all(run, "noise", "all_active")) == {1}


def test_the_traces_together_show_every_launch_site():
    seen = set()
    for setting in SETTINGS:
        seen |= {k for cr in get_run(setting).values() for k in cr.launches}
    want = T.SITES - T.SHARDED_ONLY
    assert not (want - seen), "launch sites of blockpart.hip and blocks.hip that never ran: %r" % sorted(want - seen)
    assert not (seen & T.SHARDED_ONLY), "a site of the sharded stages ran: give it a case"
