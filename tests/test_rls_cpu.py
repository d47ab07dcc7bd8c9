"""RLS-FF parameter estimator of the adaptive MPC loop (brov_rls_*, reference BLUEROV2_AMPC::RLSFF, bluerov2_ampc.cpp:731-1046)
without a GPU: known answers of the CPU restatement the kernel is held to bit for bit, the C ABI's symbols and defaults, and the
kernel's resource report (no scratch)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from rlsff_restatement import RlsffRestatement, LAM_FLOOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BROV_RLS_SYMBOLS = ["brov_rls_default_params", "brov_rls_last_error", "brov_rls_create", "brov_rls_destroy", "brov_rls_batch",
                    "brov_rls_reset", "brov_rls_set_state_host", "brov_rls_get_state_host", "brov_rls_update_host",
                    "brov_rls_update_device", "brov_rls_update_from_ekf", "brov_rls_apply_to_solver", "brov_rls_get_outputs_host",
                    "brov_rls_theta_device", "brov_rls_last_update_seconds"]


def _regressors(k, B, seed=0):
    """smooth, persistently exciting acc / vel [B][4] at tick k"""
    ph = np.random.default_rng(seed).uniform(0, 2 * np.pi, (B, 4, 3))
    t = 0.05 * k
    acc = np.sin(1.3 * t + ph[..., 0]) + 0.5 * np.sin(3.7 * t + ph[..., 1])
    vel = np.cos(0.9 * t + ph[..., 2]) + 0.3 * np.sin(2.3 * t)
    return acc, vel


def test_first_tick_is_nan_and_lambda_rises():
    B = 4
    r = RlsffRestatement(B)
    rng = np.random.default_rng(1)
    r.step(rng.normal(size=(B, 4)), rng.normal(size=(B, 4)), rng.normal(size=(B, 4)), np.zeros((B, 3)))
    assert np.isnan(r.F).all()                      # 0 / 0 over one-entry windows; NaN > 0.8 is false
    assert (r.lam == 0.9 + 0.01).all()
    assert np.isfinite(r.theta).all() and np.isfinite(r.P).all()


def test_identical_windows_give_f_one_and_lambda_falls():
    """ticks 2..5: both windows hold the same errors, so F = 1.0 exactly and lambda drops by the step each tick"""
    B = 6
    r = RlsffRestatement(B)
    rng = np.random.default_rng(2)
    lam = np.full((B, 4), 0.9 + 0.01)
    for k in range(5):
        r.step(rng.normal(size=(B, 4)) * 3, rng.normal(size=(B, 4)), rng.normal(size=(B, 4)), np.zeros((B, 3)))
        if k == 0:
            continue
        assert (r.F == 1.0).all(), k
        lam = lam - 0.01
        np.testing.assert_array_equal(r.lam, lam)
    # tick 6: the short window has dropped its first entry, the long one has not
    r.step(rng.normal(size=(B, 4)), rng.normal(size=(B, 4)), rng.normal(size=(B, 4)), np.zeros((B, 3)))
    assert not (r.F == 1.0).all()


def test_all_zero_data_keeps_f_nan_and_lambda_climbs_to_one():
    B = 3
    r = RlsffRestatement(B)
    z = np.zeros((B, 4))
    lam = []
    for _ in range(30):
        r.step(z, z, z, np.zeros((B, 3)))
        assert np.isnan(r.F).all()
        lam.append(r.lam[0, 0])
    assert max(lam) == 1.0 and lam[-1] == 1.0 and (r.lam == 1.0).all()
    k = lam.index(1.0)
    assert all(v == 1.0 for v in lam[k:]) and all(a < b for a, b in zip(lam[:k], lam[1:k + 1]))
    assert not r.theta.any()


def test_growing_error_drives_lambda_to_its_floor():
    B = 2
    r = RlsffRestatement(B)
    floor_from = None
    for k in range(150):
        acc, vel = _regressors(k, B, seed=3)
        code = r.step(np.full((B, 4), 2.0 ** k), acc, vel, np.zeros((B, 3)))
        if floor_from is None and (r.lam == 0.5).all():
            floor_from = k
        if floor_from is not None:
            assert (r.lam == 0.5).all(), k
            assert (code == LAM_FLOOR).all(), k
    assert floor_from is not None and floor_from < 100


def test_noiseless_linear_data_recovers_theta():
    """y = x . theta* with persistently exciting regressors: theta* to 1e-8 within 300 ticks (a diffuse prior P0 = 1e8 I, so that
    the prior's pull on theta is below the tolerance while lambda sits at 1)"""
    B = 8
    rng = np.random.default_rng(4)
    ts = rng.normal(size=(B, 4, 4)) * 5
    r = RlsffRestatement(B, p0=1e8)
    for k in range(300):
        acc, vel = _regressors(k, B, seed=5)
        x = [acc, vel, np.ones_like(vel), vel * np.abs(vel)]
        y = x[0] * ts[:, :, 0] + x[1] * ts[:, :, 1] + x[2] * ts[:, :, 2] + x[3] * ts[:, :, 3]
        r.step(y, acc, vel, np.zeros((B, 3)))
    assert np.abs(r.theta - ts).max() < 1e-8, np.abs(r.theta - ts).max()
    assert (r.status() == 0).all()


def test_library_exports_every_rls_symbol():
    import bluerov2_amd
    bluerov2_amd.build_library()
    lib = ctypes.CDLL(bluerov2_amd.library_path())
    missing = [n for n in BROV_RLS_SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(brov_rls_[a-z0-9_]+)\s*\(", txt)))
    assert declared == sorted(BROV_RLS_SYMBOLS)


def test_params_match_reference_defaults():
    import bluerov2_amd
    p = bluerov2_amd.RlsParams.default()
    # bluerov2_ampc.h:171-180,239-240; bluerov2_ampc.cpp:735,776-793
    assert (p.n_short, p.n_long) == (5, 50)
    assert (p.threshold, p.lambda_step, p.lambda_min, p.lambda_max, p.lambda0, p.p0, p.dt) == (0.8, 0.01, 0.5, 1.0, 0.9, 1.0, 0.05)
    assert p.compensate_coef == 0.032546960744430276 and p.rotor_constant == 0.026546960744430276
    assert ctypes.sizeof(p) == 8 + 9 * 8
    r = RlsffRestatement.from_params(2, p)
    assert (r.ns, r.nl, r.l0) == (5, 50, 0.9)


def test_no_cpu_fallback():
    import torch
    import bluerov2_amd
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(bluerov2_amd.NoDeviceError):
        bluerov2_amd.BatchRls(4)


def test_rls_kernels_use_no_scratch():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "dev", "kernel_resources.sh"), "rls_kernel.hip"], capture_output=True,
                         text=True, timeout=600).stdout
    rep = {}
    for ln in out.splitlines():
        m = re.match(r"Name: (\S+)", ln)
        if m:
            rep[m.group(1)] = {k: int(v) for k, v in re.findall(r"\|([A-Za-z ]+): (\d+)", ln)}
    names = {short: r for mangled, r in rep.items() for short in ("rls_update_kernel", "rls_inputs_kernel", "rls_apply_kernel")
             if re.search(r"\d+%sE" % short, mangled)}
    assert set(names) == {"rls_update_kernel", "rls_inputs_kernel", "rls_apply_kernel"}, sorted(rep)
    for short, r in names.items():
        assert r["scratch"] == 0, (short, r)
