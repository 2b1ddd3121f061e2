#!/usr/bin/env python3
"""Per-phase cycle breakdown of scl_decode_llr_kernel (instrumented build, -DPOLAR_PROFILE).
Run on the GPU box: python tools/phase_profile.py [L] [batch] [wpc] [lds_log]
HEAD_PHI=<leaf> (default 432, the headline code's hand-over leaf; 0 = off) also prints the share of the leaf loop's cycles spent
before that leaf: the few-path head of DESIGN.md §4.
The rate-1 block lines give the cycles of the loop iterations at positions 1 .. Z-1 of the host-marked all-unfrozen
blocks of 4 and 8 leaves whose first leaf took the fast path: the most that finishing such a block in one step could remove.
R1_OFF=1 keeps the list-of-32 kernels from finishing marked quads in one step (the marks stay: the lines above then describe the walk
without the continuation); otherwise its own cycles and its tried / committed counts are printed.
R1_RANK_OFF=1 / R1_CHAIN_OFF=1 keep the continuation from starting after a ranked first leaf / from chaining the second quad of an octet:
the two "sequel" lines then give the cycles of the loop iterations each of them would remove (profiles/r1chain)."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from polar_amd import build
lib = os.environ.get("POLAR_PROF_LIB") or build.build(profile=True)      # (an instrumented library built elsewhere)
import polar_amd
polar_amd.LIB_PATH = lib
L = int(sys.argv[1]) if len(sys.argv) > 1 else 32
B = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
wpc = int(sys.argv[3]) if len(sys.argv) > 3 else 0
ll = int(sys.argv[4]) if len(sys.argv) > 4 else 0
C.CDLL(None).srand(1)
g = polar_amd.PolarCode(11, 1024, 0.32, 16)
g.set_tuning(wpc, ll)
llr = torch.empty((B, 2048), dtype=torch.float64, device="cuda")
out = torch.empty((B, 1024), dtype=torch.uint8, device="cuda")
prof = torch.zeros(max(B, 64), dtype=torch.int64, device="cuda")
g.synth_llr_dev(1, 0, B, g.snr_sqrt_linear(float(os.environ.get("EBNO", "2.0"))), llr.data_ptr())
g.decode_scl_llr_dev(llr.data_ptr(), B, L, out.data_ptr(), prof.data_ptr())
torch.cuda.synchronize()
prof.zero_()
head_phi = int(os.environ.get("HEAD_PHI", "432"))
prof[32] = head_phi                                       # (read by the kernel: PROF_HEAD_DECL)
prof[33] = (1 if os.environ.get("R1_OFF") else 0) | (2 if os.environ.get("R1_RANK_OFF") else 0) | (4 if os.environ.get("R1_CHAIN_OFF") else 0)      # (PROF_R1_DECL)
torch.cuda.synchronize()
import time
t = time.perf_counter()
g.decode_scl_llr_dev(llr.data_ptr(), B, L, out.data_ptr(), prof.data_ptr())
torch.cuda.synchronize()
dt = time.perf_counter() - t
a = prof[:42].cpu().numpy().astype(float)
x = a[34:42]                                              # (the accumulators [32] .. [39] of the kernel: two words further up)
names = ["loop ovh", "layer S>SL g (HBM)", "layer S>SL f (HBM)", "layer 4<=S<=SL (LDS)", "layer S<4", "leaf frozen / rate-0 block", "leaf unfrozen (rest: flush etc.)", "partial sums", "unf: DPP reductions+decision", "unf: competitive-bad loop", "unf: stack/srcof", "unf: clone shuffles+update", "-", "unf: setup+goods rank loop", "unf: wait for leaf (ballot)", "unf: softplus+bounds"]
print(f"L={L} B={B} time {dt*1e3:.2f} ms -> {B/dt:.0f} cw/s")
cyc = a[:8].sum() + a[16:22].sum() + a[28]                # ([22], [23]: the head split below, not phases; [28]: the quad continuation)
nwd = B / (64 // max(1, 1 << (L - 1).bit_length()))      # wave-decodes
if os.environ.get("LATPROF"):                             # the one-codeword-per-wave kernels: a wave-decode is a codeword
    nwd = B
print(f"  cycles per wave-decode: {cyc/nwd:.0f}")
if head_phi and a[23] > 0:
    print(f"  leaves before {head_phi} (few-path head): {100*a[22]/a[23]:.2f}% of the leaf loop  {a[22]/nwd:10.0f} of {a[23]/nwd:.0f} cycles/wave-decode")
if a[25] + a[26] > 0 and a[23] > 0:
    print(f"  rate-1 blocks (marked, per wave) {a[25] + a[26]:.0f}: leaf 0 on the fast path {100*a[25]/(a[25] + a[26]):.1f}%; "
          f"later leaves of those that left it {a[27]:.0f}")
    print(f"  iterations 1..Z-1 of the blocks that started fast: {100*a[24]/a[23]:.2f}% of the leaf loop  {a[24]/nwd:10.0f} of {a[23]/nwd:.0f} cycles/wave-decode")
if a[29] > 0:
    print(f"  quad continuation (per wave): tried {a[29]:.0f}, committed {100*a[30]/a[29]:.1f}%; {100*a[28]/cyc:.1f}% of the cycles  {a[28]/nwd:10.0f} cycles/wave-decode")
if x[1] + x[3] > 0 and a[23] > 0:
    print(f"  sequel (a) iterations 1..3 of marked quads whose leaf 0 was ranked, list full: {x[1]/nwd:.1f} quads/wave-decode  "
          f"{100*x[0]/a[23]:.2f}% of the leaf loop  {x[0]/nwd:10.0f} cycles/wave-decode")
    print(f"  sequel (b) leaf-4 iterations of marked octets whose first quad was committed: {x[3]/nwd:.1f} /wave-decode  "
          f"{100*x[2]/a[23]:.2f}% of the leaf loop  {x[2]/nwd:10.0f} cycles/wave-decode")
if x[4] + x[6] > 0:
    print(f"  entry after a ranked leaf 0 (per wave-decode): tried {x[4]/nwd:.1f}, committed {x[5]/nwd:.1f}; "
          f"chain: tried {x[6]/nwd:.1f}, committed {x[7]/nwd:.1f}")
for nm, v in zip(names[:8], a[:8]):
    print(f"  {nm:34s} {100*v/cyc:5.1f}%  {v/nwd:10.0f} cycles/wave-decode")
sub = ["unf: leaf wait + softplus + DPP bounds", "unf: fast path commit", "unf: goods rank loop", "unf: competitive-bad loop",
       "unf: kill/clone LIFO (LDS)", "unf: clone shuffles + update", "-", "-"]
for nm, v in zip(sub, a[16:22]):
    if v:
        print(f"    {nm:40s} {100*v/cyc:5.1f}%  {v/nwd:10.0f}")
if a[8] > 0:
    print(f"  unfrozen steps (per wave) {a[8]:.0f}: fast path {100*a[9]/a[8]:.1f}%, full-list ranking {100*a[10]/a[8]:.1f}%")
    if a[10] > 0:
        print(f"  per ranking step: competitive bad forks (union over groups) {a[11]/a[10]:.2f}, contested good forks {a[12]/a[10]:.2f}")
        print(f"  per ranking step: surviving bad forks (max over groups) {a[13]/a[10]:.2f}; steps with <= 4: {100*a[14]/a[10]:.1f}%, with none: {100*a[15]/a[10]:.1f}%")
