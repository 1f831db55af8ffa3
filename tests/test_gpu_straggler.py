"""The shared straggler model (csrc/straggler.h) on the host and on the
device: the two must agree bit for bit, and both must agree with
engine/delay.py wherever Python's half-to-even round() and C's
half-away-from-zero round() cannot differ (docs/TESTING.md)."""

import math

import numpy as np
import pytest
import torch  # noqa: F401  first, as everywhere: _hip_core shares its HIP runtime

pytestmark = pytest.mark.gpu

from asyncframework_amd import _hip_core
from asyncframework_amd.engine.delay import DelayInjector
from asyncframework_amd.utils.philox import uniform01

SEED = 42
COEFFS = (-1.0, 0.0, 1.0, 2.5)
ROUNDS = (0, 3, 17, 2 ** 31 + 5)


def _pairs(P):
    wid = [w for w in range(P) for _ in ROUNDS]
    rk = [r for _ in range(P) for r in ROUNDS]
    return wid, rk


def _host(P, coeff, avg, wid, rk):
    return [_hip_core.straggler_delay_probe(P, coeff, SEED, avg, w, r)
            for w, r in zip(wid, rk)]


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def test_host_and_device_probe_agree_bitwise():
    """Every P in 1..64, every wid: one one-thread launch per
    (P, coeff, avg)."""
    nonzero = 0
    for P in range(1, 65):
        wid, rk = _pairs(P)
        for coeff in COEFFS:
            for avg in (100.0, 3.7, 0.0):
                host = _host(P, coeff, avg, wid, rk)
                dev = _hip_core.straggler_delay_probe_device(
                    P, coeff, SEED, avg, wid, rk)
                assert len(dev) == len(host)
                bad = np.nonzero(_bits(host) != _bits(dev))[0]
                assert bad.size == 0, (P, coeff, avg, wid[bad[0]],
                                       rk[bad[0]], host[bad[0]],
                                       dev[bad[0]])
                nonzero += sum(1 for h in host if h != 0.0)
    assert nonzero > 1000  # the comparison was not of zeros alone


def _unrounded(inj, wid, rk):
    """The product delay_ms() rounds, or None where it returns 0.0."""
    if inj.coeff == 0.0:
        return None
    if not inj.cloud:
        return inj.coeff * inj.avg_delay_ms if wid == 0 and inj.coeff > 0 \
            else None
    if wid in inj.straggler_longtail:
        u = float(uniform01(inj.seed, rk, wid, 1)[0])
        return (u * 7.5 + 2.5) * inj.avg_delay_ms
    if wid in inj.straggler_normal:
        u = float(uniform01(inj.seed, rk, wid, 1)[0])
        return (u + 1.5) * inj.avg_delay_ms
    return None


def test_both_probes_match_python_injector():
    """P where both rounding rules select the same straggler sets; products
    within 1e-9 of a .5 tie are left out (the two round() rules may differ
    there), and they are rare."""
    total = excluded = 0
    for P in (4, 8, 12, 16, 32):
        wid, rk = _pairs(P)
        for coeff in COEFFS:
            for avg in (100.0, 3.7):
                inj = DelayInjector(P, coeff=coeff, seed=SEED,
                                    calib_window=0)
                inj._cul_time, inj._cul_count = avg, 1
                inj.maybe_activate(1)
                assert inj.avg_delay_ms == avg
                host = _host(P, coeff, avg, wid, rk)
                dev = _hip_core.straggler_delay_probe_device(
                    P, coeff, SEED, avg, wid, rk)
                for i, (w, r) in enumerate(zip(wid, rk)):
                    total += 1
                    x = _unrounded(inj, w, r)
                    if x is not None and \
                            abs(x - math.floor(x) - 0.5) < 1e-9:
                        excluded += 1
                        continue
                    ref = inj.delay_ms(w, r)
                    assert host[i] == ref, (P, coeff, avg, w, r)
                    assert dev[i] == ref, (P, coeff, avg, w, r)
    assert excluded < 0.01 * total, (excluded, total)
