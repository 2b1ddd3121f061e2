"""Rates of the systematic precode and message kernels beside encode_dev, the cost of the message step behind a decode, the host table
build time and the BER gain -> profiles/sys/rates.json.

Device-resident, the headline code N = 2048, K = 1024, CRC 16. Variants on the same rows, alternated inside one process:
  encode                 encode_dev (the plain encoder: one wave per codeword, bytes in LDS), info [B][K] -> coded [B][N];
  precode_u              encode_systematic_dev, msg -> u_info [B][K] alone;
  precode                encode_systematic_dev, msg -> coded [B][N] and u_info;
  message                systematic_message_dev, u_info -> msg [B][K]
at B = 65 536; then decode_scl_llr_dev alone and followed by the message step, L = 1 at B = 262 144 and L = 32 at B = 65 536 (rows at
Eb/N0 2.0 dB). One warm-up round, `--rounds` timed rounds of `--calls` back-to-back calls between HIP events; median [min - max].
The spread of a variant is (max - min) / median over its rounds; the tool states it and holds the message kernel to the encoder's
rate within it. Beside the rates: the wall time of the host table build (polar_get_sys_info on a fresh handle) at n = 11 and n = 15,
and systematic_stats beside get_bler_quick's BER on the plain code at 1.5, 2.0, 2.5 dB for L = 1 and 8.
The measurements run in a child process under a time limit; a failed child ends the run.

    python tools/sys_rates.py [--out profiles/sys/rates.json] [--rounds 5] [--calls 4]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CODE = (11, 1024, 16)
B_KERNELS = 65536
DECODES = ((1, 262144), (32, 65536))
RATE_EBNO = 2.0
EBNO_POINTS = (1.5, 2.0, 2.5)
BER_LISTS = (1, 8)
LIMIT = 900          # seconds


def summary(xs):
    med = statistics.median(xs)
    return {"median": med, "min": min(xs), "max": max(xs), "spread": (max(xs) - min(xs)) / med, "rounds": xs}


def timed(variants, call, rounds, calls, B):
    """{variant: summary of M rows / s}: round 0 warms up, the variants alternate inside every round."""
    import torch
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rate = {v: [] for v in variants}
    for r in range(rounds + 1):
        for v in variants:
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(calls):
                call(v)
            ev1.record()
            torch.cuda.synchronize()
            if r:
                rate[v].append(calls * B / (ev0.elapsed_time(ev1) * 1e-3) / 1e6)
    return {k: summary(x) for k, x in rate.items()}


def one(rounds, calls, max_runs, max_err):
    import ctypes as C
    import torch
    import polar_amd
    n, K, crc = CODE
    N = 1 << n
    torch.cuda.set_device(0)
    res = {"code": list(CODE), "table_build_s": {}}
    for nn in (11, 15):                                    # the first systematic call of a fresh handle builds the tables
        C.CDLL(None).srand(C.c_uint(1))
        h = polar_amd.PolarCode(nn, 1 << (nn - 1), 0.32, 16)
        t0 = time.perf_counter()
        depth, swapped = h.systematic_info()
        res["table_build_s"][str(nn)] = {"seconds": time.perf_counter() - t0, "depth": depth, "n_swapped": swapped}
        h.close()
    C.CDLL(None).srand(C.c_uint(1))
    g = polar_amd.PolarCode(n, K, 0.32, crc)
    Bmax = max(B_KERNELS, max(b for _, b in DECODES))
    gen = torch.Generator(device="cuda").manual_seed(3)
    msg = torch.randint(0, 2, (B_KERNELS, K), dtype=torch.uint8, device="cuda", generator=gen)
    u = torch.zeros((B_KERNELS, K), dtype=torch.uint8, device="cuda")
    back = torch.zeros((B_KERNELS, K), dtype=torch.uint8, device="cuda")
    coded = torch.zeros((B_KERNELS, N), dtype=torch.uint8, device="cuda")

    def kernel_call(v):
        if v == "encode":
            g.encode_dev(msg.data_ptr(), B_KERNELS, coded.data_ptr())
        elif v == "precode_u":
            g.encode_systematic_dev(msg.data_ptr(), B_KERNELS, 0, u.data_ptr())
        elif v == "precode":
            g.encode_systematic_dev(msg.data_ptr(), B_KERNELS, coded.data_ptr(), u.data_ptr())
        else:
            g.systematic_message_dev(u.data_ptr(), B_KERNELS, back.data_ptr())

    res["kernels_Mcw_s"] = timed(["encode", "precode_u", "precode", "message"], kernel_call, rounds, calls, B_KERNELS)
    res["round_trip_ok"] = bool((back == msg).all())
    k = res["kernels_Mcw_s"]
    tol = max(k["message"]["spread"], k["encode"]["spread"])
    res["message_vs_encode"] = {"ratio": k["message"]["median"] / k["encode"]["median"], "spread": tol,
                                "holds": bool(k["message"]["median"] >= k["encode"]["median"] * (1 - tol))}
    # the message step behind a decode
    llr = torch.empty((Bmax, N), dtype=torch.float64, device="cuda")
    out = torch.zeros((Bmax, K), dtype=torch.uint8, device="cuda")
    g.synth_sys_llr_dev(7, 0, Bmax, g.snr_sqrt_linear(RATE_EBNO), llr.data_ptr())
    res["decode_Mcw_s"] = {}
    for L, B in DECODES:
        def decode_call(v, L=L, B=B):
            g.decode_scl_llr_dev(llr.data_ptr(), B, L, out.data_ptr())
            if v == "decode+message":
                g.systematic_message_dev(out.data_ptr(), B, out.data_ptr())
        d = timed(["decode", "decode+message"], decode_call, rounds, max(1, calls // 2), B)
        d["added_share"] = d["decode"]["median"] / d["decode+message"]["median"] - 1
        res["decode_Mcw_s"]["L%d,B%d" % (L, B)] = d
    # BER: the systematic code beside the plain one on the same trials
    pts = list(EBNO_POINTS)
    s = g.systematic_stats(pts, BER_LISTS, max_runs=max_runs, max_err=max_err, seed=11)
    bler, ber = g.get_bler_quick(pts, BER_LISTS, max_runs=max_runs, max_err=max_err, seed=11, return_ber=True)
    res["ber_ebno_db"], res["ber_lists"] = pts, list(BER_LISTS)
    res["systematic"] = {"bler": s["bler"].tolist(), "ber_msg": s["ber_msg"].tolist(), "ber_u": s["ber_u"].tolist(),
                         "stats": s["stats"].tolist()}
    res["plain_get_bler_quick"] = {"bler": bler.tolist(), "ber_per_run_over_K": (ber / K).tolist()}
    print("SYS " + json.dumps(res), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sys", "rates.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--max-runs", type=int, default=100000)
    ap.add_argument("--max-err", type=int, default=200)
    ap.add_argument("--one", action="store_true", help="the measurements themselves (a child of this tool)")
    a = ap.parse_args()
    if a.one:
        return one(a.rounds, a.calls, a.max_runs, a.max_err)
    from polar_amd import build
    build.build()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--rounds", str(a.rounds), "--calls", str(a.calls),
                            "--max-runs", str(a.max_runs), "--max-err", str(a.max_err)], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print("sys_rates: exceeded its time limit of %d s; stopping" % LIMIT, file=sys.stderr)
        return 124
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("SYS ")]
    if r.returncode != 0 or not line:
        print("sys_rates: failed (exit %d)\n%s" % (r.returncode, r.stderr[-2000:]), file=sys.stderr)
        return r.returncode or 1
    res = json.loads(line[-1][4:])
    for name, row in res["kernels_Mcw_s"].items():
        print("%-10s %8.2f [%8.2f - %8.2f] M codewords / s, spread %.1f %%" % (name, row["median"], row["min"], row["max"], 100 * row["spread"]))
    print("message / encode = %.2f (spread %.1f %%): %s" % (res["message_vs_encode"]["ratio"], 100 * res["message_vs_encode"]["spread"],
                                                           "holds" if res["message_vs_encode"]["holds"] else "DOES NOT HOLD"))
    for name, d in res["decode_Mcw_s"].items():
        print("%s: decode %.3f, decode + message %.3f M codewords / s (+%.2f %% time)" %
              (name, d["decode"]["median"], d["decode+message"]["median"], 100 * d["added_share"]))
    print("table build:", json.dumps(res["table_build_s"]))
    print("systematic:", json.dumps({k2: res["systematic"][k2] for k2 in ("bler", "ber_msg", "ber_u")}))
    print("plain:", json.dumps(res["plain_get_bler_quick"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"tool": "tools/sys_rates.py", "rounds": a.rounds, "calls_per_round": a.calls,
               "clock": "HIP events around the back-to-back device-resident calls; M codewords / s",
               "ber_stop": {"max_runs": a.max_runs, "max_err": a.max_err}, "result": res}, open(a.out, "w"), indent=1)
    print("wrote", a.out)
    return 0 if res["message_vs_encode"]["holds"] and res["round_trip_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
