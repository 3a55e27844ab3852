"""Every path of the DBSCAN engine (csrc/dbscan.hip) against the CPU oracle, bit for bit, with proof from the library's own
trace (VCP_TRACE) that the path meant is the path that ran: the case table of tests/engine_path_cases.py, once under the
default switches and once under every developer switch of dbscan.hip, gridbuild.hip and the block pipeline -- the source
says of them "None changes a result, only the path that computes it", and tools/gpu/ab.sh benchmarks them against each
other on that promise.

The switches are read once per process, so every setting is a fresh child (tests/_engine_paths_worker.py) that runs the
whole table; VCP_TRACE=1 and the switch are the only VCP_* variables it sees.  For every case the child compares labels,
is_core, is_classed, cf and evals with the oracle; the parent holds the launches traced between the case's markers to the
case's expectation (the sites that must appear, the sites that must not, the values on the `vcp-trace dbscan` line) and
checks that the switch took effect somewhere -- a switch that silently does nothing fails.  The children run one after
another; if one ends by signal, abort or time limit, no further child is started and the remaining tests fail at once,
naming it."""
import os
import subprocess
import sys

import pytest

import engine_path_cases as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_engine_paths_worker.py")
CHILD_TIMEOUT = 120  # seconds; a child needs its start-up and about three seconds

SETTINGS = {
    "default": {},
    "no_screen": {"VCP_NO_SCREEN": "1"},
    "no_lists": {"VCP_NO_LISTS": "1"},
    "core_cap_0": {"VCP_CORE_CAP": "0"},
    "core_cap_1": {"VCP_CORE_CAP": "1"},
    "core_cap_15": {"VCP_CORE_CAP": "15"},
    "core_global": {"VCP_CORE_GLOBAL": "1"},
    "join_all_0": {"VCP_JOIN_ALL": "0"},
    "join_all_1": {"VCP_JOIN_ALL": "1"},
    "cell_budget_1": {"VCP_CELL_BUDGET": "1"},
    "part_pairs_0": {"VCP_PART_PAIRS": "0"},
    "noise_all": {"VCP_NOISE_ALL": "1"},
    "blocks_order_sort": {"VCP_BLOCKS_ORDER_SORT": "1"},
    "brute_max_0": {"VCP_BRUTE_MAX": "0"},
}
# what a setting changes in the model of the driver (engine_path_cases.sites) ...
SITE_SWITCH = {"no_lists": dict(lists=False), "core_global": dict(core_global=True), "join_all_0": dict(join_all=0),
               "join_all_1": dict(join_all=1)}
# ... and which values of the `vcp-trace dbscan` line it moves away from what a case wants by default
MOVED = {"no_lists": {"NB", "core_cap", "dense", "join_all"}, "core_cap_0": {"core_cap"}, "core_cap_1": {"core_cap"},
         "core_cap_15": {"core_cap"}, "join_all_0": {"join_all"}, "join_all_1": {"join_all"},
         "cell_budget_1": {"cellw", "ncells"}}
PAIRS, NO_PAIRS = "(k_part_scatter_pairs<GD, GROUPED>)", "(k_part_scatter<GD, GROUPED>)"

_runs, _fatal = {}, []


class CaseRun:
    def __init__(self):
        self.status, self.launches, self.lines, self.events = None, [], [], []  # events: launches and lines in order

    def engine_lines(self):
        """the `vcp-trace dbscan` lines of the calls that reached the grid path"""
        return [d for what, d in self.lines if what == "dbscan" and "_words" not in d]

    def words(self, what, word):
        return [d for w, d in self.lines if w == what and d.get("_words") == [word]]

    def core_kernels(self):
        """[(the `vcp-trace dbscan` line of a grid call, the core-count kernel launched for it)]"""
        out, last = [], None
        for what, payload in self.events:
            if what == "launch" and payload in (T.CORE_LDS, T.CORE_GLOBAL):
                last = payload
            elif what == "dbscan" and "_words" not in payload:
                out.append((payload, last))
        return out


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
            what, payload = T.parse_trace_line(line)
            cur.events.append((what, payload))
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
    try:
        p = subprocess.run([sys.executable, WORKER], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        tail = (e.stderr or b"")[-1500:]
        _fatal.append("the child of setting %s ran into its time limit of %d s:\n%s" % (
            setting, CHILD_TIMEOUT, tail.decode(errors="replace") if isinstance(tail, bytes) else tail))
        pytest.fail(_fatal[0])
    if p.returncode not in (0, 1):
        _fatal.append("the child of setting %s ended with status %d:\n%s\n%s" % (setting, p.returncode, p.stdout[-1000:],
                                                                                 p.stderr[-3000:]))
        pytest.fail(_fatal[0])
    run = parse(p.stderr)
    missing = [c.name for c in T.CASES if c.name not in run or run[c.name].status is None]
    assert not missing, "cases without a result: %r\n%s" % (missing[:5], p.stderr[-2000:])
    _runs[setting] = run
    return run


def check_case(case, cr, setting):
    """-> list of complaints about one case under one setting"""
    bad = []
    if cr.status != "ok":
        bad.append("differs from the oracle: " + cr.status)
    must, must_not = case.expect(**SITE_SWITCH.get(setting, {}))
    if case.kind == "blocks":  # the pipeline's second engine call (the noise points, not grouped) counts through k_core_lds
        must_not = must_not - {T.CORE_LDS}
    seen = set(cr.launches) & T.SITES
    if must - seen:
        bad.append("launch sites missing from the trace: %r" % sorted(must - seen))
    if seen & must_not:
        bad.append("launch sites that must not run: %r" % sorted(seen & must_not))
    early = case.params.get("early")
    lines = cr.engine_lines()
    if early:
        if lines or len(cr.words("dbscan", early)) != 1:
            bad.append("expected one `vcp-trace dbscan %s` line and no grid call" % early)
        return bad
    if case.kind == "engine" and len(lines) != 1:
        bad.append("%d `vcp-trace dbscan` lines for one engine call" % len(lines))
    if case.kind == "slabs":
        lines = [d for d in lines if d["slab"] == 1]
        if len(lines) != 2:
            bad.append("%d staged engine calls for two ranks" % len(lines))
    if case.kind == "blocks":
        lines = [d for d in lines if d["grouped"] == 1]
        if not lines:
            bad.append("no grouped engine call")
    moved = MOVED.get(setting, set())
    for d in lines:
        for key, want in case.want.items():
            if key in moved:
                continue
            ok = want(d) if callable(want) else d.get(key) == want
            if not ok:
                bad.append("the trace line does not show %s%s: %r" % (key, "" if callable(want) else " == %r" % (want,), d))
    return bad


def check_table(setting):
    run = get_run(setting)
    bad = []
    for case in T.CASES:
        bad += ["%s: %s" % (case.name, b) for b in check_case(case, run[case.name], setting)]
    assert not bad, "%d complaints under %s:\n%s" % (len(bad), setting, "\n".join(bad[:40]))
    return run


def all_engine_lines(run):
    return [(name, d) for name, cr in run.items() for d in cr.engine_lines()]


def test_default():
    run = check_table("default")
    lines = all_engine_lines(run)
    # what the switch tests below compare against
    assert any(d["screen"] == 1 for _, d in lines) and any(d["NB"] == 15 for _, d in lines)
    assert {d["join_all"] for _, d in lines} == {0, 1} and {d["dense"] for _, d in lines} == {0, 1}
    assert {d["part_out"] for _, d in lines} == {0, 1}
    assert any(d["core_cap"] < d["NB"] for _, d in lines), "no list cut to core_cap"
    g = run["grouped_blocks"]
    assert g.words("blocks", "partition")[0]["brute_thr"] == 1024 and g.words("blocks", "noise")[0]["all_active"] == 0
    assert g.words("blocks", "order")[0]["by_sort"] == 0
    scat = [d for cr in run.values() for w, d in cr.lines if w == "gridbuild"]
    assert scat and all(d["stash"] == 1 for d in scat)
    launches = {k for cr in run.values() for k in cr.launches}
    assert PAIRS in launches and NO_PAIRS not in launches


def test_no_screen():
    lines = all_engine_lines(check_table("no_screen"))
    assert lines and all(d["screen"] == 0 and d["sc.lo"] == -1 and d["sc.hi"] == float("inf") for _, d in lines)


def test_no_lists():
    run = check_table("no_lists")
    assert all(d["NB"] == 0 for _, d in all_engine_lines(run))
    launches = {k for cr in run.values() for k in cr.launches}
    assert "k_union_init_list" not in launches and T.BORDER_LIST not in launches


@pytest.mark.parametrize("cap", [0, 1, 15])
def test_core_cap(cap):
    run, base = check_table("core_cap_%d" % cap), get_run("default")
    lines = all_engine_lines(run)
    assert all(d["core_cap"] == min(d["NB"], cap) for _, d in lines)
    was = {name: [d["core_cap"] for d in base[name].engine_lines()] for name in base}
    assert any([d["core_cap"] for d in run[name].engine_lines()] != was[name] for name in run), "the switch moved nothing"


def test_core_global():
    run = check_table("core_global")  # (the table's expectation for the grouped case is k_core under this switch)
    for which, kernel in (("core_global", T.CORE_GLOBAL), ("default", T.CORE_LDS)):
        calls = get_run(which)["grouped_blocks"].core_kernels()
        grouped = [k for d, k in calls if d["grouped"] == 1]
        assert grouped and set(grouped) == {kernel}, "%s: the grouped call counted through %r" % (which, grouped)
        assert all(k == T.CORE_LDS for d, k in calls if d["grouped"] == 0), "the switch is for grouped calls only"
    assert all(k == (T.CORE_LDS if d["gd"] == 2 else T.CORE_GLOBAL) for name, cr in run.items() if name != "grouped_blocks"
               for d, k in cr.core_kernels())


@pytest.mark.parametrize("every", [0, 1])
def test_join_all(every):
    run, base = check_table("join_all_%d" % every), get_run("default")
    flipped = set()
    for case in T.CASES:
        if case.kind != "engine" or not case.params["lists"] or case.params.get("early"):
            continue
        d, d0 = run[case.name].engine_lines()[0], base[case.name].engine_lines()[0]
        assert d["join_all"] == every, case.name
        if d0["join_all"] != every:
            flipped.add(case.params["regime"])
            assert ("k_flatten0<2>" if every else "k_flatten0<1>") in run[case.name].launches
            assert ("k_flatten0<1>" if every else "k_flatten0<2>") in base[case.name].launches
    assert flipped == ({"lt"} if every else {"ge", "dense"}), flipped


def test_cell_budget():
    run, base = check_table("cell_budget_1"), get_run("default")
    d, d0 = run["budget_l1"].engine_lines()[0], base["budget_l1"].engine_lines()[0]
    assert d0["ncells"] > 65536 and d0["cellw"] < 1.01
    assert d["ncells"] <= 65536 and d["cellw"] > 1.2, "VCP_CELL_BUDGET=1 did not coarsen the grid: %r" % d


def test_part_pairs_off():
    run = check_table("part_pairs_0")
    scat = [d for cr in run.values() for w, d in cr.lines if w == "gridbuild"]
    assert scat and all(d["pairs_on"] == 0 and d["stash"] == 0 for d in scat)
    launches = {k for cr in run.values() for k in cr.launches}
    assert NO_PAIRS in launches and PAIRS not in launches


def test_noise_all():
    g = check_table("noise_all")["grouped_blocks"]
    assert g.words("blocks", "noise")[0]["all_active"] == 1


def test_blocks_order_sort():
    g = check_table("blocks_order_sort")["grouped_blocks"]
    assert g.words("blocks", "order")[0]["by_sort"] == 1


def test_brute_max_0():
    g = check_table("brute_max_0")["grouped_blocks"]
    assert g.words("blocks", "partition")[0]["brute_thr"] == 0


def test_the_traces_together_show_every_launch_site():
    seen = set()
    for setting in SETTINGS:
        seen |= {k for cr in get_run(setting).values() for k in cr.launches}
    assert not (T.SITES - seen), "launch sites of dbscan.hip that never ran: %r" % sorted(T.SITES - seen)
