"""The Gaussian-approximation construction through the two other host surfaces: the MEX gateway command 'ga_design' (driven
through the mx / mex runtime of tests/mex_runtime/ the way polar_amd/matlab/PolarCode.m's ga_code_construction drives it,
as tests/test_mex_gateway.py does for the other commands) and PolarCode::ga_code_construction of the C++ mirror
(polar_amd/cpp/PolarCode.hpp, compiled into a small program). Both must give the Python layer's code bit for bit."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IDS = ['ask4-gray', 'ask8-gray', 'ask16-gray', 'bpsk', 'ask4-sp', 'ask8-sp', 'ask16-sp']   # PolarCode.m: find(...) = POLAR_CONST_*


@pytest.fixture(scope="module")
def mex(built_lib):
    import fake_matlab
    return fake_matlab.polar_mex()


def _ga_m(pc, design_snr_db, constellation_name='bpsk', receiver_algo='bicm', phi_dx=1e-5, seed=1, capacity=None):
    """polar_amd/matlab/PolarCode.m ga_code_construction, call for call (fake_matlab.PolarCodeM's conventions)."""
    cid = IDS.index(constellation_name) + 1
    if receiver_algo == 'mlc':
        cid += 256
    cap = np.zeros((0,)) if capacity is None else np.asarray(capacity, np.float64)
    old = pc.h
    pc.h, fz, order0, est, channels = pc.mex('ga_design', pc.n, pc.info_length, pc.crc_size, pc.crc_matrix.astype(np.uint8), cid,
                                             design_snr_db, phi_dx, seed, cap, nlhs=5)
    pc.mex('destroy', old, nlhs=0)
    pc.frozen_bits = fz.astype(np.float64)
    pc.info_bits = order0.reshape(-1)[:pc.info_length + pc.crc_size].astype(np.float64) + 1
    pc.channels = channels.reshape(-1)
    pc.cc_method, pc.cc_parameter, pc.cc_misc = 'gauss-approx', design_snr_db, f"{constellation_name}_{receiver_algo}"
    return float(est[0, 0])


@pytest.mark.parametrize("snr,name,rx,crc,cap", [(2.5, "bpsk", "bicm", 0, None), (9.0, "ask4-gray", "bicm", 8, None),
                                                 (14.0, "ask16-sp", "mlc", 0, None),
                                                 (12.0, "ask16-gray", "bicm", 0, [0.02, 0.3, 0.1, 0.9])])
def test_gateway_ga_design(mex, snr, name, rx, crc, cap):
    import fake_matlab
    import polar_amd
    pc = fake_matlab.PolarCodeM(1024, 512, 0.32, crc)
    est = _ga_m(pc, snr, name, rx, 1e-5, 3, cap)
    want = polar_amd.PolarCode.from_gauss_approx(1024, 512, snr, name, rx, crc, pc.crc_matrix.astype(np.uint8) if crc else None,
                                                 1e-5, 3, cap)
    assert est == want.bler_estimate
    assert (pc.channels == want.channels).all()
    assert (pc.frozen_bits[0] == want.frozen_bits).all()
    order = np.argsort(-want.channels, kind="stable")
    assert (pc.info_bits - 1 == order[:512 + crc]).all()
    if crc == 0:
        assert (pc.decode_scl_llr(np.full(1024, 3.0), 8) == 0).all()       # the new handle decodes (all-zero codeword)
    pc.delete()


def test_gateway_ga_design_refuses(mex):
    import fake_matlab
    pc = fake_matlab.PolarCodeM(1024, 512, 0.32, 0)
    with pytest.raises(fake_matlab.MexError) as e:
        _ga_m(pc, 3.0, 'ask8-gray')
    assert e.value.identifier == "polar_amd:error"
    with pytest.raises(fake_matlab.MexError):
        mex('ga_design', 10.0, 2000.0, 0.0, np.zeros((0,), np.uint8), 4.0, 3.0, 1e-5, 1.0)     # K > N
    pc.delete()


CPP = r'''
#include <cstdio>
#include <cstdlib>
#include "PolarCode.hpp"
int main(int argc, char **argv) {
    // argv: n K crc constellation snr
    const int n = atoi(argv[1]), K = atoi(argv[2]), crc = atoi(argv[3]), c = atoi(argv[4]);
    PolarCode pc((uint8_t)n, (uint16_t)K, 0.32, (uint16_t)crc);
    const double est = pc.ga_code_construction(atof(argv[5]), c);
    std::vector<double> p1(1u << n, 0.05);
    std::vector<double> u = pc.decode_sc_p1(p1);
    int zeros = 0;
    for (double v : u) zeros += v == 0.0;
    printf("%.17g %d\n", est, zeros);
    for (double v : pc.channels()) printf("%.17g\n", v);
    return 0;
}
'''


def test_cpp_mirror_ga_code_construction(built_lib, tmp_path):
    import polar_amd
    from polar_amd import build
    src = tmp_path / "ga_cpp.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "ga_cpp")
    here = os.path.dirname(built_lib)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(build.ROOT, "include"), "-I", os.path.join(here, "cpp"),
                           str(src), "-o", exe, "-L", here, "-lpolar_amd", "-Wl,-rpath," + here,
                           "-Wl,-rpath," + (build._torch_lib() or "/opt/rocm/lib"), "-Wl,-rpath,/opt/rocm/lib"])
    for n, K, crc, c, rx, snr in ((10, 512, 0, 4, "bicm", 2.5), (10, 500, 12, 7, "mlc", 14.0)):
        name = IDS[c - 1]
        out = subprocess.run([exe, str(n), str(K), str(crc), str(c | (256 if rx == "mlc" else 0)), str(snr)],
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.split("\n")
        est, zeros = lines[0].split()
        ch = np.array([float(v) for v in lines[1:1 + (1 << n)]])
        want = polar_amd.PolarCode.from_gauss_approx(1 << n, K, snr, name, rx, crc,
                                                     np.zeros((crc, K), np.uint8) if crc else None)
        assert float(est) == want.bler_estimate
        assert (ch == want.channels).all()
        assert int(zeros) == K                                              # all-zero codeword decoded by the new handle
