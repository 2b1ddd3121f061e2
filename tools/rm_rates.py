"""Rates of the rate-matching recover kernel beside a device-to-device copy, the cost of recover in front of a decode, and a short
BLER table of the three E < N schemes -> profiles/rm/rates.json.

Device-resident, N = 2048, K = 768, CRC 16, B = 65 536, designs of PolarCode.from_gauss_approx_rm at 1.5 dB.
  recover   rate_recover_dev at E = 1536 (puncture, shorten: f64 and f16 rows; NR's scattered pattern: f64, reported apart) and E = 3072
            (repeat, f64) beside hipMemcpyAsync device-to-device of B N 8 bytes (what recover writes), alternated inside every round;
            milliseconds per call. For E <= N recover moves at most the bytes that copy reads and writes: the tool holds it to the
            copy's time within the spread it observes between rounds.
  decode    decode_scl_llr_rm_dev on the received rows beside decode_scl_llr_dev in mode 1 on the rows already recovered (the
            difference is what recover adds), and beside the automatic-mode decode of mother-code rows at the same B (what the
            dispatch rule costs), L = 1, 8, 32; M codewords / s.
  sweep     rm_stats at Eb/N0 1.5, 2.0, 2.5 dB, L = 1 and 8, shorten / puncture / NR (for the record).
One warm-up round, `--rounds` timed rounds of `--calls` back-to-back calls between HIP events; median [min - max].

    python tools/rm_rates.py [--out profiles/rm/rates.json] [--rounds 5] [--calls 4]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_LOG2, K, CRC = 11, 768, 16
B = 65536
DESIGN_EBNO = 1.5
LISTS = (1, 8, 32)
EBNO_POINTS = (1.5, 2.0, 2.5)
BLER_LISTS = (1, 8)


def summary(xs):
    med = statistics.median(xs)
    return {"median": med, "min": min(xs), "max": max(xs), "spread": (max(xs) - min(xs)) / med, "rounds": xs}


def timed(variants, call, rounds, calls):
    """{variant: summary of ms per call}: round 0 warms up, the variants alternate inside every round."""
    import torch
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {v: [] for v in variants}
    for r in range(rounds + 1):
        for v in variants:
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(calls):
                call(v)
            ev1.record()
            torch.cuda.synchronize()
            if r:
                ms[v].append(ev0.elapsed_time(ev1) / calls)
    return {k: summary(x) for k, x in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rm", "rates.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--max-runs", type=int, default=20000)
    ap.add_argument("--max-err", type=int, default=100)
    a = ap.parse_args()
    import numpy as np
    import torch
    import polar_amd
    torch.cuda.set_device(0)
    N = 1 << N_LOG2
    hip = C.CDLL("libamdhip64.so")
    stream = torch.cuda.current_stream().cuda_stream
    codes = {s: polar_amd.PolarCode.from_gauss_approx_rm(N, K, E, s, DESIGN_EBNO, CRC)
             for s, E in (("puncture", 1536), ("shorten", 1536), ("nr", 1536), ("repeat", 3072))}
    res = {"code": [N_LOG2, K, CRC], "B": B, "weak_leaves": {s: g.weak_leaves for s, g in codes.items()}}

    # ---- recover beside the copy ----
    llr = torch.empty((B, N), dtype=torch.float64, device="cuda")
    src = torch.randn((B, N), dtype=torch.float64, device="cuda")
    rx = {}
    for s, g in codes.items():
        E = g.rate_match_info()[0].size
        rx[s, "f64"] = torch.randn((B, E), dtype=torch.float64, device="cuda")
        if s in ("puncture", "shorten"):
            rx[s, "f16"] = rx[s, "f64"].to(torch.float16)
    variants = ["copy"] + ["%s/%s" % k for k in rx]

    def recover_call(v):
        if v == "copy":
            assert hip.hipMemcpyAsync(C.c_void_p(llr.data_ptr()), C.c_void_p(src.data_ptr()), C.c_size_t(B * N * 8), C.c_int(3), C.c_void_p(stream)) == 0
            return
        s, fmt = v.split("/")
        codes[s].rate_recover_dev(rx[s, fmt].data_ptr(), fmt, B, llr.data_ptr())
    rec = timed(variants, recover_call, a.rounds, a.calls)
    for v, row in rec.items():
        if v == "copy":
            row["bytes"] = 2 * B * N * 8
        else:
            s, fmt = v.split("/")
            row["bytes"] = B * N * 8 + rx[s, fmt].numel() * rx[s, fmt].element_size()
        row["GB_per_s"] = row["bytes"] / (row["median"] * 1e-3) / 1e9
    tol = max(r["spread"] for r in rec.values())
    res["recover_ms"] = rec
    res["recover_vs_copy"] = {v: {"ratio": rec[v]["median"] / rec["copy"]["median"], "spread": tol,
                                  "holds": bool(rec[v]["median"] <= rec["copy"]["median"] * (1 + tol))}
                              for v in variants if v.split("/")[0] in ("puncture", "shorten")}
    del src

    # ---- recover in front of a decode ----
    g = codes["shorten"]
    E = 1536
    out = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    mother = torch.empty((B, N), dtype=torch.float64, device="cuda")
    g.synth_rm_llr_dev(1, 0, B, g.snr_sqrt_linear_rm(2.0), rx["shorten", "f64"].data_ptr())
    g.rate_recover_dev(rx["shorten", "f64"].data_ptr(), "f64", B, llr.data_ptr())
    g.synth_llr_dev(1, 0, B, g.snr_sqrt_linear(2.0), mother.data_ptr())
    res["decode_Mcw_per_s"] = {}
    for L in LISTS:
        def decode_call(v, L=L):
            if v == "rm":
                g.decode_scl_llr_rm_dev(rx["shorten", "f64"].data_ptr(), "f64", B, L, out.data_ptr())
            elif v == "mode1_recovered":
                g.set_mode(1)
                g.decode_scl_llr_dev(llr.data_ptr(), B, L, out.data_ptr())
                g.set_mode(0)
            else:
                g.decode_scl_llr_dev(mother.data_ptr(), B, L, out.data_ptr())
        t = timed(("rm", "mode1_recovered", "auto_mother"), decode_call, a.rounds, a.calls)
        row = {v: summary([B / (x * 1e-3) / 1e6 for x in t[v]["rounds"]]) for v in t}
        row["recover_adds"] = t["rm"]["median"] / t["mode1_recovered"]["median"] - 1
        row["rule_costs"] = t["mode1_recovered"]["median"] / t["auto_mother"]["median"]
        res["decode_Mcw_per_s"]["L%d" % L] = row

    # ---- a short BLER table ----
    res["bler"] = {}
    for s in ("shorten", "puncture", "nr"):
        st = codes[s].rm_stats(list(EBNO_POINTS), list(BLER_LISTS), a.max_runs, a.max_err, seed=1)
        res["bler"][s] = {"ebno_db": list(EBNO_POINTS), "lists": list(BLER_LISTS), "bler": st["bler"].tolist(), "ber": st["ber"].tolist(),
                          "runs": st["stats"][:, :, polar_amd.RM_RUN].tolist()}

    for v, row in rec.items():
        print("%-14s %7.3f [%7.3f - %7.3f] ms, %6.0f GB/s, spread %.1f %%" % (v, row["median"], row["min"], row["max"], row["GB_per_s"], 100 * row["spread"]))
    for v, row in res["recover_vs_copy"].items():
        print("%-14s %.3f of the copy's time (spread %.1f %%): %s" % (v, row["ratio"], 100 * row["spread"], "holds" if row["holds"] else "DOES NOT HOLD"))
    for Lk, row in res["decode_Mcw_per_s"].items():
        print("%-4s rm %.3f, mode 1 on recovered rows %.3f, automatic on mother rows %.3f M cw/s; recover adds %.1f %%, the rule costs x%.2f" %
              (Lk, row["rm"]["median"], row["mode1_recovered"]["median"], row["auto_mother"]["median"], 100 * row["recover_adds"], row["rule_costs"]))
    for s, row in res["bler"].items():
        print(s, np.array(row["bler"]).round(5).tolist())
    res["method"] = {"rounds": a.rounds, "calls": a.calls, "clock": "HIP events around back-to-back device-resident calls on one stream",
                     "warmup": "one untimed round", "variants": "alternated inside every round"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
