"""The pipelined-round schedule of get_bler_quick (polar_amd/csrc/polar_mc_schedule.h) on a CPU: tests/mc_schedule_main.cpp
drives McSchedule with a fake error model and prints every step; here the same model runs through the plain round-after-round
loop of polar_amd/montecarlo.py (next_round, enabled = err <= max_err decided per round, every enabled point simulated,
run += T), and the two must agree — the claim of the header's comment, without a GPU."""
import collections
import os
import subprocess

import pytest

from polar_amd.montecarlo import next_round

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "mc_schedule_main.cpp")
INC = os.path.join(ROOT, "polar_amd", "csrc")

# (n_e, n_L, max_runs, max_err, batch, parts)
PIPELINED = ((20, 200, 3000), (5, 64, 2000), (0, 100, 700), (40, 0, 5000), (10**6, 333, 2000))   # test_gpu_montecarlo.py's tuples
CASES = [(5, 3, max_runs, max_err, batch, parts) for max_err, batch, max_runs in PIPELINED for parts in (1, 3)] + [
    (1, 1, 1000, 10, 100, 1),        # one point, one list size: two slots
    (1, 1, 1000, 0, 100, 1),
    (5, 3, 1001, 20, 200, 2),        # max_runs no multiple of batch: a short last round
    (4, 2, 1500, 0, 128, 1),         # max_err = 0: a point stops with its first error
    (5, 3, 20000, 40, 0, 8),         # geometric rounds over 8 devices
    (3, 2, 300000, 1000, 0, 8),
]


def fake_errors(base, T, li, ie):
    """mc_schedule_main.cpp fake_errors."""
    shift = 2 * ie + li
    return min(T, ((T >> shift) if shift < 62 else 0) + (1 if (base + li + ie) % 3 == 0 else 0))


def _compile(out, extra=()):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", INC, SRC, "-o", out, *extra], capture_output=True, text=True)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mc_schedule") / "mc_schedule_main")
    r = _compile(out)           # (the header alone: no ROCm include path is given)
    assert r.returncode == 0, r.stderr
    return out


def run_schedule(exe, case):
    """-> (steps, err, run, done, rounds); steps = [(admitted T, done, rounds, [(li, ie, slot, T, base, fresh), ...]), ...]"""
    r = subprocess.run([exe] + [str(v) for v in case], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (case, r.stdout[-400:], r.stderr[-2000:])
    steps, err, run, end = [], None, None, None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "step":
            steps.append((int(w[3]), int(w[5]), int(w[7]), []))
        elif w[0] == "stage":
            steps[-1][3].append(tuple(int(x) for x in w[1:]))
        elif w[0] == "end":
            end = (int(w[2]), int(w[4]))
        elif w[0] in ("err", "run"):
            vals = [int(x) for x in w[1:]]
            err, run = (vals, run) if w[0] == "err" else (err, vals)
    assert end is not None and err is not None and run is not None, r.stdout[-400:]
    return steps, err, run, end[0], end[1]


def round_after_round(n_e, n_L, max_runs, max_err, batch, parts):
    """polar_amd/montecarlo.py get_bler_quick_sharded with the fake model as its engine -> (err, run, simulated, round sizes)"""
    P = n_e * n_L
    err, run, sim, sizes = [0] * P, [0] * P, collections.Counter(), []
    base = 0
    while base < max_runs:
        T = next_round(batch, max_err, base, max_runs, parts)
        enabled = [e <= max_err for e in err]                    # PolarCode.cpp:725, once per round
        if not any(enabled):
            break
        for li in range(n_L):
            for ie in range(n_e):
                if enabled[li * n_e + ie]:
                    sim[(base, T, li, ie)] += 1
                    err[li * n_e + ie] += fake_errors(base, T, li, ie)
                    run[li * n_e + ie] += T
        base += T
        sizes.append(T)
    return err, run, sim, sizes


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_schedule_equals_the_round_after_round_loop(exe, case):
    n_e, n_L, max_runs, max_err, batch, parts = case
    steps, err, run, done, rounds = run_schedule(exe, case)
    want_err, want_run, want_sim, want_sizes = round_after_round(*case)
    # final totals, and what was simulated (each (round, list size, point) at most once)
    assert err == want_err and run == want_run
    sim = collections.Counter((base, T, li, ie) for _, _, _, st in steps for li, ie, slot, T, base, fresh in st)
    assert sim == want_sim
    # termination: the rounds of the loop (a round started while the last points were about to stop may follow them: the multiset
    # above says it simulates nothing), their sizes by next_round, no trial beyond max_runs
    sizes = [a for a, _, _, _ in steps if a]
    assert sizes[:len(want_sizes)] == want_sizes
    assert sizes == [next_round(batch, max_err, sum(sizes[:i]), max_runs, parts) for i in range(len(sizes))]
    assert rounds == len(sizes) and done == sum(sizes) <= max_runs
    assert all(d <= max_runs for _, d, _, _ in steps)
    seen, last_at, first_step, last_step, slot_of = set(), {}, {}, {}, {}
    for k, (_, _, _, st) in enumerate(steps):
        for li in range(n_L):
            mine = [s for s in st if s[0] == li]
            # order inside a step: oldest round first, strictly downwards in the points, one stage per round
            assert all(a[4] < b[4] and a[1] > b[1] for a, b in zip(mine, mine[1:])), (k, mine)
        for li, ie, slot, T, base, fresh in st:
            assert 0 <= ie < n_e and 0 <= slot <= n_e
            # fresh exactly on the first stage of a (round, list size)
            assert bool(fresh) == ((base, li) not in seen), (k, base, li)
            seen.add((base, li))
            # no round overtakes the one before it: a point sees the rounds in their order, each in a later step than the last;
            # and a round moves upwards through its points
            pk, pbase = last_at.get(("point", li, ie), (-1, -1))
            assert k > pk and base > pbase, (k, li, ie, base)
            last_at[("point", li, ie)] = (k, base)
            rk, rie = last_at.get(("round", li, base), (-1, -1))
            assert k > rk and ie > rie, (k, li, ie, base)
            last_at[("round", li, base)] = (k, ie)
            first_step.setdefault(base, k)
            last_step[base] = k
            assert slot_of.setdefault(base, slot) == slot
    # slots: rounds in flight at the same time (first to last stage) never share one, and there are at most n_e + 1 of them
    bases = sorted(first_step)
    assert [slot_of[b] for b in bases] == [i % (n_e + 1) for i in range(len(bases))]
    for k in range(len(steps)):
        live = [b for b in bases if first_step[b] <= k <= last_step[b]]
        assert len(live) <= n_e + 1 and len({slot_of[b] for b in live}) == len(live), (k, live)


def test_schedule_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same program, stand-alone, built with -fsanitize=address,undefined: one case with early stops and a short last round."""
    out = str(tmp_path / "mc_schedule_main_san")
    r = _compile(out, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ cannot link the sanitizer runtimes: " + r.stderr.strip().splitlines()[-1][:200])
    assert r.returncode == 0, r.stderr
    case = (5, 3, 3001, 20, 200, 3)
    _, err, run, _, _ = run_schedule(out, case)
    want_err, want_run, _, _ = round_after_round(*case)
    assert err == want_err and run == want_run
