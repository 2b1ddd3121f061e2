"""One handle through every kernel family of decode_scl_llr in turn, and back: the families share the handle's scratch (the
per-wave state buffers, the flag and work-list buffers, the work counter), so a launcher that sized or filled them for itself
alone shows only in a sequence. Every result is compared bit for bit with the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, K = 1024, 512


def test_families_in_sequence_on_one_handle(built_lib, oracle_built):
    import ctypes as C
    import torch
    import polar_amd
    from oracle_lib import Oracle
    o = Oracle(10, K, 0.32, 8, srand=1)
    C.CDLL(None).srand(C.c_uint(1))
    g = polar_amd.PolarCode(10, K, 0.32, 8)
    llr, _ = o.synth_llr(77, 0, 70, o.snr_sqrt_linear(1.5))
    p1 = 1.0 / (1.0 + np.exp(llr[:3]))
    want = {L: o.decode_scl_llr(llr[:B], L) for L, B in ((1, 70), (2, 5), (4, 5), (8, 9), (32, 40))}
    want_pm = [o.decode_scl_llr_pm(llr[i], 1)[1] for i in range(3)]
    want_p1 = np.stack([o.decode_scl_p1(p1[i], 1.0 - p1[i], 4) for i in range(3)])
    want_sc = np.stack([o.decode_sc_p1(p1[i]) for i in range(3)])

    buf = torch.zeros(70 * N + 1, dtype=torch.float64, device="cuda")
    rows = {off: buf[off: off + 70 * N] for off in (0, 1)}          # rows at a 16-byte aligned address / 8 bytes further
    out = torch.empty((70, K), dtype=torch.uint8, device="cuda")
    pm = torch.empty(70, dtype=torch.float64, device="cuda")
    cand = torch.empty((9, 8, K), dtype=torch.uint8, device="cuda")
    win = torch.empty(9, dtype=torch.int32, device="cuda")

    def dev(L, B, off=0, lat=0, with_pm=False, waves_per_cu=0):
        def run():
            rows[off].copy_(torch.from_numpy(llr.reshape(-1)))
            assert rows[off].data_ptr() % 16 == 8 * off
            g.debug_set("lat_max_b", lat)
            g.set_tuning(waves_per_cu=waves_per_cu)
            out.zero_()
            g.decode_scl_llr_dev(rows[off].data_ptr(), B, L, out.data_ptr(), pm_ptr=pm.data_ptr() if with_pm else 0)
            torch.cuda.synchronize()
            g.set_tuning()
            g.debug_set("lat_max_b", 0)
            assert (out[:B].cpu().numpy() == want[L][:B]).all()
            if with_pm:
                got = pm[:B].cpu().numpy()
                assert all(abs(got[i] - want_pm[i]) <= 1e-10 * max(1.0, abs(want_pm[i])) for i in range(B)), (got, want_pm)
        return run

    def list_winners():
        rows[0].copy_(torch.from_numpy(llr.reshape(-1)))
        g.decode_scl_llr_list_dev(rows[0].data_ptr(), "f64", 9, 8, cand.data_ptr(), winner_ptr=win.data_ptr())
        torch.cuda.synchronize()
        c, w = cand.cpu().numpy(), win.cpu().numpy()
        got = np.stack([c[b, w[b]] if w[b] >= 0 else np.zeros(K, np.uint8) for b in range(9)])
        assert (got == want[8]).all()

    def scl_p1():
        assert (g.decode_scl_p1(p1, 1.0 - p1, 4) == want_p1).all()

    def sc_p1():
        assert (g.decode_sc_p1(p1) == want_sc).all()

    calls = [dev(1, 3), dev(1, 3, with_pm=True), dev(1, 70, off=1), dev(1, 70, lat=-1), dev(2, 5), dev(4, 5), dev(4, 5, lat=-1),
             dev(32, 40),                          # the small-batch geometry
             dev(32, 40, waves_per_cu=16),         # the default geometry, table mode
             list_winners, scl_p1, sc_p1]
    for i, call in enumerate(calls + calls[::-1]):
        try:
            call()
        except AssertionError as e:
            raise AssertionError("call %d of the sequence (1-based %d of the list)" % (i, min(i, 23 - i) + 1)) from e
