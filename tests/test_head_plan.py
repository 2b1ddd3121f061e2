"""The plan of the two-phase list decode (polar_amd/csrc/polar_head_plan.h) on a CPU: tests/head_plan_main.cpp prints head_plan()
for a frozen mask; here the same quantities are restated from the walk of the list kernel — which leaf writes a layer, which
reads it — and the values DESIGN.md §3 lists for the Bhattacharyya codes (eps = 0.32) are pinned."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "head_plan_main.cpp")
INC = os.path.join(ROOT, "polar_amd", "csrc")
FIELDS = ("phi_h", "paths", "t", "window", "llr_mask", "c_mask", "llr_rows", "c_rows", "rows", "record_words")


def _compile(out, extra=()):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", INC, SRC, "-o", out, *extra], capture_output=True, text=True)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("head_plan") / "head_plan_main")
    r = _compile(out)           # (the header alone: no ROCm include path is given)
    assert r.returncode == 0, r.stderr
    return out


def prefix_params(frozen):
    """polar_decode.cpp prefix_params for groups of 4 lanes and more -> (Q, Pe)"""
    N = len(frozen)
    P = 0
    while P < N and frozen[P]:
        P += 1
    if P >= 256:
        Q = 256
    else:
        Q = 64
        while Q <= P:
            Q <<= 1
        if P < 33:
            Q = 0
    if Q > N // 2:
        Q = 0
    return Q, (min(P, Q) if Q else 0)


def run_plan(exe, frozen, Q, Pe, cap, decision=None):
    n = len(frozen).bit_length() - 1
    args = [exe, str(n), str(Q), str(Pe), str(cap), "".join("1" if f else "0" for f in frozen)]
    if decision:
        args += [str(int(v)) for v in decision]
    r = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    w = lines[0].split()
    plan = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}
    assert tuple(plan) == FIELDS
    if decision:
        plan["use"] = int(lines[1].split()[1])
        # head_record_ok: the row the plan asks for passes; each of the eight ways to flip one active bit or miscount one word does not
        assert lines[2].split() == ["record_ok", "1", "caught", "8"], lines[2]
    return plan


def walk_plan(frozen, Q, Pe, cap):
    """The same plan from the kernel's walk, leaf by leaf: the layer of T elements is written by the visit at every leaf that is a
    multiple of T and read (as the input of the layer below) at every leaf that is a multiple of T/2; column 0 of the partial sums
    of the layer of S elements is written when a left child of S leaves is complete and read until its sibling is."""
    N = len(frozen)
    n = N.bit_length() - 1
    unf = [i for i in range(N) if not frozen[i]][:3]
    none = dict(phi_h=0, paths=0, t=0, window=0, llr_mask=0, c_mask=0, llr_rows=0, c_rows=0, rows=3, record_words=12)
    if Q <= 0 or N < 64 or len(unf) < 3:
        return none
    phi = unf[2] // 16 * 16
    if phi >= cap:
        phi = (cap - 1) // 16 * 16
    if phi <= Pe or phi <= 0:
        return none
    t = sum(1 for u in unf[:2] if u < phi)
    llr_mask = c_mask = llr_rows = c_rows = 0
    for s in range(5, n):
        T = 1 << s
        if T >= Q and phi < T:
            continue                      # still read from the prefix pass's buffer
        nxt = next(q for q in range(phi, phi + 2 * T + 1) if q % (T // 2) == 0)      # first visit from phi on that touches the layer
        if nxt % T != 0:                  # ... reads it (a multiple of T rewrites it first)
            llr_mask |= 1 << s
            llr_rows += T
    for s in range(6, n):
        S = 1 << s
        if (phi // S) % 2 == 1:           # inside a right child of S leaves: the left one's decisions are waiting
            c_mask |= 1 << s
            c_rows += S // 32
    rows = 3 + c_rows + llr_rows
    return dict(phi_h=phi, paths=1 << t, t=t, window=phi - Pe, llr_mask=llr_mask, c_mask=c_mask, llr_rows=llr_rows, c_rows=c_rows,
                rows=rows, record_words=4 * rows)


def mask(N, unfrozen):
    f = np.ones(N, np.uint8)
    f[list(unfrozen)] = 0
    return f


# (n, K, crc) -> phi_h, paths, window, live LLR layers, live partial-sum layers (0 = the head is not taken)
CODES = {
    (11, 1024, 16): (432, 4, 177, (32, 128), (128, 256)),
    (11, 512, 16): (496, 1, 240, (32,), (64, 128, 256)),
    (12, 2048, 16): (752, None, 496, None, None),
    (10, 256, 8): (368, None, 113, None, None),
    (9, 128, 8): (208, None, 81, None, None),
    (10, 512, 16): (None, None, 17, None, None),
}


@pytest.mark.parametrize("code", sorted(CODES), ids=lambda c: "-".join(str(v) for v in c))
def test_plan_of_the_bhattacharyya_codes(exe, oracle_built, code):
    from oracle_lib import Oracle
    n, K, crc = code
    frozen = Oracle(n, K, 0.32, crc).frozen()
    Q, Pe = prefix_params(frozen)
    N = 1 << n
    got = run_plan(exe, frozen, Q, Pe, N // 2)
    assert got == walk_plan(frozen, Q, Pe, N // 2)
    phi_h, paths, window, llr_layers, c_layers = CODES[code]
    assert got["window"] == window
    if phi_h is not None:
        assert got["phi_h"] == phi_h
    if paths is not None:
        assert got["paths"] == paths
    if llr_layers is not None:
        assert got["llr_mask"] == sum(llr_layers) and got["llr_rows"] == sum(llr_layers)
        assert got["c_mask"] == sum(c_layers) and got["c_rows"] == sum(c_layers) // 32
    if code == (11, 1024, 16):
        # the first unfrozen leaves, and the record: 160 doubles and 12 partial-sum words per path, 5.5 KiB per codeword
        assert [i for i in range(N) if not frozen[i]][:6] == [255, 383, 439, 443, 445, 446]
        assert got["rows"] == 175 and got["record_words"] * 8 == 5600
    # the decision: the default tuning, a batch that fills the device, a window of 64 leaves
    use = lambda **kw: run_plan(exe, frozen, Q, Pe, N // 2, decision=[kw.get(k, d) for k, d in
                                (("tuning", 1), ("B", 65536), ("min_b", 65536), ("off", 0))])["use"]
    assert use() == (1 if window >= 64 else 0)
    assert use(tuning=0) == 0 and use(B=65535) == 0 and use(off=1) == 0
    assert use(B=1, min_b=1) == (1 if window >= 64 else 0)


def test_no_prefix_pass_no_head(exe, oracle_built):
    from oracle_lib import Oracle
    frozen = Oracle(11, 1800, 0.32, 16).frozen()
    Q, Pe = prefix_params(frozen)
    assert Q == 0
    got = run_plan(exe, frozen, Q, Pe, 1024, decision=(1, 1 << 20, 1, 0))
    assert got["phi_h"] == 0 and got["paths"] == 0 and got["use"] == 0


def test_cap(exe):
    """A third unfrozen leaf at or beyond the cap: the largest multiple of 16 below it (N/4 and N/2 of N = 2048)."""
    frozen = mask(2048, [300, 700, 1500] + list(range(1600, 2048)))
    for cap, want in ((512, 496), (1024, 1008), (2048, 1488), (1488, 1472), (1489, 1488)):
        got = run_plan(exe, frozen, 256, 256, cap)
        assert got == walk_plan(frozen, 256, 256, cap)
        assert got["phi_h"] == want and got["phi_h"] < cap
        assert got["t"] == sum(1 for u in (300, 700) if u < want) and got["paths"] == 1 << got["t"]
    # capped at or below the resume point: nothing left to hand over
    assert run_plan(exe, frozen, 256, 256, 272)["phi_h"] == 0
    assert run_plan(exe, frozen, 256, 256, 273)["phi_h"] == 272


@pytest.mark.parametrize("unfrozen", [(), (700,), (300, 2047)], ids=("none", "one", "two"))
def test_fewer_than_three_unfrozen_leaves(exe, unfrozen):
    got = run_plan(exe, mask(2048, unfrozen), 256, 256, 1024)
    assert got["phi_h"] == 0 and got["paths"] == 0 and got["rows"] == 3


@pytest.mark.parametrize("third", [448, 512, 272, 1008])
def test_third_unfrozen_leaf_on_a_multiple_of_16(exe, third):
    """The hand-over leaf is then that leaf itself: four paths arrive and the 32-lane kernel takes the fork."""
    frozen = mask(2048, [260, third - 1, third] + list(range(third + 5, 2048)))
    got = run_plan(exe, frozen, 256, 256, 1024)
    assert got == walk_plan(frozen, 256, 256, 1024)
    assert got["phi_h"] == third and got["paths"] == 4 and got["t"] == 2 and got["window"] == third - 256


def test_random_masks_against_the_walk(exe):
    rng = np.random.default_rng(5)
    for _ in range(60):
        n = int(rng.integers(7, 13))
        N = 1 << n
        first = int(rng.integers(33, N // 2))
        frozen = np.ones(N, np.uint8)
        frozen[first:] = rng.random(N - first) < rng.choice([0.5, 0.9, 0.98])
        frozen[first] = 0
        Q, Pe = prefix_params(frozen)
        for cap in (N // 4, N // 2):
            assert run_plan(exe, frozen, Q, Pe, cap) == walk_plan(frozen, Q, Pe, cap), (n, first, cap)


def test_plan_under_address_and_undefined_behaviour_sanitizers(tmp_path, oracle_built):
    """The same program, stand-alone, built with -fsanitize=address,undefined, on the headline code's mask."""
    from oracle_lib import Oracle
    out = str(tmp_path / "head_plan_main_san")
    r = _compile(out, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert r.returncode == 0, r.stderr          # (the sanitizer runtimes are part of the toolchain this suite needs: no skip)
    frozen = Oracle(11, 1024, 0.32, 16).frozen()
    got = run_plan(out, frozen, 256, 255, 1024, decision=(1, 65536, 65536, 0))
    assert got["phi_h"] == 432 and got["use"] == 1
    assert run_plan(out, mask(128, [40, 41]), 64, 40, 64)["phi_h"] == 0
