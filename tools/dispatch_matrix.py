#!/usr/bin/env python3
"""tools/dispatch_matrix.py — does a change of the host dispatch launch what the build before it launched?

    rocprofv3 --kernel-trace --output-format csv -d <dir A> -- python tools/dispatch_matrix.py run --lib <library A>
    rocprofv3 --kernel-trace --output-format csv -d <dir B> -- python tools/dispatch_matrix.py run
    python tools/dispatch_matrix.py compare <dir A> <dir B> > profiles/refactor/dispatch_trace.txt

`run` makes a fixed matrix of calls on ONE handle of the N = 1024 code (10, 512, 8) — every kernel family of decode_scl_llr
through the device-resident entry points (the twelve calls of tests/test_gpu_dispatch_sequence.py), one pipelined host batch,
one short get_bler_quick and the variants of the list decoder (adaptive, host-pointer list output in chunks, path metric, the two
sweeps) — and prints one line per call. `compare` reads the two kernel traces in the order of submission
and compares kernel name, grid, workgroup and LDS size dispatch by dispatch; exit status 1 if they differ.
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(lib_path):
    import numpy as np
    import torch
    import polar_amd
    if lib_path:
        polar_amd.use_library(lib_path)
    N, K = 1024, 512
    g = polar_amd.PolarCode(10, K, 0.32, 8)
    buf = torch.zeros(70 * N, dtype=torch.float64, device="cuda")
    g.synth_llr_dev(77, 0, 70, g.snr_sqrt_linear(1.5), buf.data_ptr())
    shifted = torch.zeros(70 * N + 1, dtype=torch.float64, device="cuda")          # the same rows, 8 bytes off a 16-byte boundary
    shifted[1:].copy_(buf)
    rows = (buf.data_ptr(), shifted.data_ptr() + 8)
    out = torch.empty((70, K), dtype=torch.uint8, device="cuda")
    pm = torch.empty(70, dtype=torch.float64, device="cuda")
    cand = torch.empty((9, 8, K), dtype=torch.uint8, device="cuda")
    win = torch.empty(9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    llr = buf.cpu().numpy().reshape(70, N)
    p1 = 1.0 / (1.0 + np.exp(llr[:3]))

    def dev(L, B, off=0, lat=0, with_pm=False, waves_per_cu=0):
        g.debug_set("lat_max_b", lat)
        g.set_tuning(waves_per_cu=waves_per_cu)
        g.decode_scl_llr_dev(rows[off], B, L, out.data_ptr(), pm_ptr=pm.data_ptr() if with_pm else 0)
        torch.cuda.synchronize()
        g.set_tuning()
        g.debug_set("lat_max_b", 0)
        print("dev L=%d B=%d offset=%d lat_max_b=%d pm=%d waves_per_cu=%d" % (L, B, 8 * off, lat, with_pm, waves_per_cu))

    for kw in (dict(L=1, B=3), dict(L=1, B=3, with_pm=True), dict(L=1, B=70, off=1), dict(L=1, B=70, lat=-1), dict(L=2, B=5),
               dict(L=4, B=5), dict(L=4, B=5, lat=-1), dict(L=32, B=40), dict(L=32, B=40, waves_per_cu=16)):
        dev(**kw)
    g.decode_scl_llr_list_dev(buf.data_ptr(), "f64", 9, 8, cand.data_ptr(), winner_ptr=win.data_ptr())
    torch.cuda.synchronize()
    print("list L=8 B=9")
    g.decode_scl_p1(p1, 1.0 - p1, 4)
    print("decode_scl_p1 L=4 B=3")
    g.decode_sc_p1(p1)
    print("decode_sc_p1 B=3")
    g.debug_set("host_pipe_min_bytes", 1)
    g.debug_set("host_chunk_bytes", 16 * N * 8)
    g.debug_set("host_lanes", 1)          # (one lane: one stream, so the order of the dispatches is the order of submission)
    g.decode_scl_llr(llr, 4)
    print("host batch L=4 B=70 chunks=%d" % g.debug_get("host_chunks"))
    for key in ("host_pipe_min_bytes", "host_chunk_bytes", "host_lanes"):
        g.debug_set(key, 0)
    bler = g.get_bler_quick([1.0, 2.0], [1, 4], max_runs=2000, max_err=20, seed=3)
    print("get_bler_quick", bler.tolist())
    # the variants of the list decoder: adaptive, the host-pointer list call over a chunk boundary, the path metric, their sweeps
    g.decode_scl_llr_adaptive_dev(buf.data_ptr(), "f64", 9, (1, 4, 32), out.data_ptr())
    torch.cuda.synchronize()
    print("adaptive schedule=(1, 4, 32) B=9")
    g.debug_set("list_chunk_cw", 5)
    lists = g.decode_scl_llr_list(llr[:9], 8)
    print("host list L=8 B=9 list_chunk_cw=5")
    g.path_metric(llr[:9], lists[0])
    print("path_metric B=9 R=8")
    g.debug_set("list_chunk_cw", 7)
    stats = np.zeros((2, 2, polar_amd.LS_N), np.uint64)
    g.mc_batch_list(3, 0, 23, 1, [1.0, 2.0], [2, 8], np.ones((2, 2), np.uint8), stats)
    print("mc_batch_list T=23 L=(2, 8) list_chunk_cw=7", stats[:, :, :2].tolist())
    stats = np.zeros((2, polar_amd.AD_STAGE0 + 3), np.uint64)
    g.mc_batch_adaptive(3, 0, 23, 1, [1.0, 2.0], (1, 4, 32), np.ones(2, np.uint8), stats)
    print("mc_batch_adaptive T=23 schedule=(1, 4, 32) list_chunk_cw=7", stats.tolist())
    g.debug_set("list_chunk_cw", 0)


def dispatches(d):
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[-1]
    rows = list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r.get("Correlation_Id") or r["Dispatch_Id"]))

    def dims(r, stem):
        return tuple(int(r[stem + a]) for a in "_X _Y _Z".split()) if stem + "_X" in r else (int(r[stem]),)
    return [(r["Kernel_Name"], dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), int(r["LDS_Block_Size"])) for r in rows]


def compare(a, b):
    da, db = dispatches(a), dispatches(b)
    same = sum(1 for x, y in zip(da, db) if x == y)
    print("kernel dispatches: %d before, %d after; %d equal in name, grid, workgroup and LDS size, position by position" % (len(da), len(db), same))
    for i, (x, y) in enumerate(zip(da, db)):
        if x != y:
            print("first difference at dispatch %d:\n  before %s\n  after  %s" % (i, x, y))
            break
    print("\n%6s  %-14s %-12s %7s  kernel" % ("count", "grid", "workgroup", "LDS"))
    seen = {}
    for x in da:
        seen[x] = seen.get(x, 0) + 1
    for (name, grid, wg, lds), n in seen.items():          # (in the order of first use)
        print("%6d  %-14s %-12s %7d  %s" % (n, "x".join(map(str, grid)), "x".join(map(str, wg)), lds, name[:110]))
    ok = da == db
    print("\nresult: %s" % ("IDENTICAL" if ok else "DIFFERENT"))
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run(sys.argv[3] if len(sys.argv) > 3 and sys.argv[2] == "--lib" else None)
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
