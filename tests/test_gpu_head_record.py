"""The premise of the two-phase list decode, checked on what the head really leaves (the test build of the library: polar_debug_get
"head_check" reads row 2 of every hand-over record back and holds it against the plan, polar_head_plan.h head_record_ok): every
codeword arrives with exactly 1 << t paths, in the top lanes of the 4-list, t unfrozen leaves decided — no path was killed in the
head, at any of the hand-overs the GPU tests use."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CODES = {(11, 1024, 16): 432, (11, 512, 16): 496, (10, 256, 8): 368, (9, 128, 8): 208}


@pytest.mark.parametrize("code", sorted(CODES), ids=lambda c: "-".join(str(v) for v in c))
def test_records_hold_the_planned_paths(hooks_lib, oracle_built, code):
    import torch
    import polar_amd
    n, K, crc = code
    C.CDLL(None).srand(C.c_uint(1))
    g = polar_amd.PolarCode(n, K, 0.32, crc)
    assert g.debug_get("test_hooks") == 1
    g.set_tuning(waves_per_cu=16)
    g.debug_set("head_min_b", 1)
    assert g.debug_get("head_check") == -2                       # nothing decoded yet
    B = 50
    llr = torch.empty((B, 1 << n), dtype=torch.float64, device="cuda")
    out = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    for L in (32, 17):
        g.synth_llr_dev(7, 0, B, g.snr_sqrt_linear(0.5), llr.data_ptr())
        g.decode_scl_llr_dev(llr.data_ptr(), B, L, out.data_ptr())
        torch.cuda.synchronize()
        assert g.debug_get("head_phi") == CODES[code]
        assert g.debug_get("head_check") == 0
    g.debug_set("no_head", 1)
    g.decode_scl_llr_dev(llr.data_ptr(), B, 32, out.data_ptr())
    torch.cuda.synchronize()
    assert g.debug_get("head_check") == -2                       # one phase: no records
