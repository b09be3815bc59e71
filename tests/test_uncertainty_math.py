"""The positional-uncertainty math (dynadjust_amd/csrc/uncertainty.h) through its host entry dnagpu_debug_uncertainty_3x3 (no device):
local covariance, 1-sigma error ellipse, azimuth convention and the SP1 95 % figures, against an independent numpy restatement and
against the exact 95 % radius of a bivariate normal."""
import ctypes as C
import math

import numpy as np
import pytest

from dynadjust_amd import _lib

SP1 = (1.960790, 0.004071, 0.114276, 0.371625)


def device_math(lib, c6, lat, lon):
    out = _lib.DnaGpuUncertainty()
    arr = (C.c_double * 6)(*[float(v) for v in c6])
    lib.dnagpu_debug_uncertainty_3x3(arr, float(lat), float(lon), C.byref(out))
    return np.array(list(out.enu)), out.semi_major, out.semi_minor, out.azimuth, out.hz_pu, out.vt_pu


def rotation(lat, lon):
    """columns: east, north, up in cartesian axes"""
    sl, cl, so, co = math.sin(lat), math.cos(lat), math.sin(lon), math.cos(lon)
    return np.array([[-so, -sl * co, cl * co], [co, -sl * so, cl * so], [0.0, cl, sl]])


def full(c6):
    xx, xy, xz, yy, yz, zz = c6
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def reference(c6, lat, lon):
    """numpy restatement: eigen-decomposition of the horizontal block, azimuth from the major eigenvector"""
    R = rotation(lat, lon)
    Q = R.T @ full(c6) @ R
    w, v = np.linalg.eigh(Q[:2, :2])
    a, b = math.sqrt(max(w[1], 0.0)), math.sqrt(max(w[0], 0.0))
    ve, vn = v[0, 1], v[1, 1]
    az = math.atan2(ve, vn) % math.pi
    c = b / a if a > 0 else 0.0
    hz = a * (SP1[0] + SP1[1] * c + SP1[2] * c * c + SP1[3] * c ** 3)
    return Q[np.triu_indices(3)], a, b, az, hz, 1.96 * math.sqrt(Q[2, 2])


def az_diff(x, y):
    d = abs(x - y) % math.pi
    return min(d, math.pi - d)


def test_random_spd_matches_numpy(built):
    rng = np.random.default_rng(20261015)
    for _ in range(500):
        M = rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-3, -1)
        S = M @ M.T + np.eye(3) * 1e-8
        c6 = S[np.triu_indices(3)]
        lat, lon = rng.uniform(-math.pi / 2, math.pi / 2), rng.uniform(-math.pi, math.pi)
        enu, a, b, az, hz, vt = device_math(built, c6, lat, lon)
        renu, ra, rb, raz, rhz, rvt = reference(c6, lat, lon)
        scale = np.abs(S).max()
        assert np.abs(enu - renu).max() <= 1e-13 * scale
        assert abs(a - ra) <= 1e-13 * ra
        assert abs(b - rb) <= 1e-12 * ra
        assert abs(hz - rhz) <= 1e-12 * rhz
        assert abs(vt - rvt) <= 1e-13 * rvt
        assert 0.0 <= az < math.pi
        if (ra - rb) > 1e-3 * ra:            # (the azimuth of a nearly circular ellipse is ill-conditioned)
            assert az_diff(az, raz) < 1e-9


# at lat = lon = 0 the local frame is exact: east = +Y, north = +Z, up = +X, so ee = C_yy, nn = C_zz, en = C_yz
def at_origin(ee, nn, en, uu=1.0):
    return [uu, 0.0, 0.0, ee, en, nn]


@pytest.mark.parametrize("ee,nn,en,expected", [
    (4.0, 1.0, 0.0, math.pi / 2),         # along east
    (1.0, 4.0, 0.0, 0.0),                 # along north
    (2.0, 2.0, 1.0, math.pi / 4),         # north-east
    (2.0, 2.0, -1.0, 3 * math.pi / 4),    # south-east / north-west
])
def test_azimuth_axes(built, ee, nn, en, expected):
    _, a, b, az, _, _ = device_math(built, at_origin(ee, nn, en), 0.0, 0.0)
    assert abs(az - expected) < 1e-15
    assert a > b


@pytest.mark.parametrize("ee,nn,en,lo,hi", [
    (1.0, 3.0, 0.5, 0.0, math.pi / 4),                 # first quadrant, nearer north
    (3.0, 1.0, 0.5, math.pi / 4, math.pi / 2),         # first quadrant, nearer east
    (3.0, 1.0, -0.5, math.pi / 2, 3 * math.pi / 4),    # second quadrant, nearer east
    (1.0, 3.0, -0.5, 3 * math.pi / 4, math.pi),        # second quadrant, nearer north
])
def test_azimuth_quadrants(built, ee, nn, en, lo, hi):
    c6 = at_origin(ee, nn, en)
    _, _, _, az, _, _ = device_math(built, c6, 0.0, 0.0)
    assert lo < az < hi
    assert az_diff(az, reference(c6, 0.0, 0.0)[3]) < 1e-14


def test_circle_and_rank_deficient(built):
    enu, a, b, az, hz, vt = device_math(built, at_origin(2.0, 2.0, 0.0, uu=9.0), 0.0, 0.0)
    assert az == 0.0 and a == b == math.sqrt(2.0)
    assert hz == pytest.approx(a * sum(SP1), rel=1e-15)
    assert vt == pytest.approx(1.96 * 3.0, rel=1e-15)
    # horizontal part of rank one: b = 0, c = 0
    enu, a, b, az, hz, vt = device_math(built, at_origin(1.0, 4.0, 2.0), 0.0, 0.0)
    assert b == 0.0 and a == pytest.approx(math.sqrt(5.0), rel=1e-15)
    assert hz == pytest.approx(a * SP1[0], rel=1e-15)
    # nothing at all
    enu, a, b, az, hz, vt = device_math(built, [0.0] * 6, 0.3, 0.4)
    assert (a, b, az, hz, vt) == (0.0, 0.0, 0.0, 0.0, 0.0)


def exact_radius95(a, b):
    """radius of the circle holding 95 % of N(0, diag(a^2, b^2)): P(r) = int phi_a(x) P(|y| <= sqrt(r^2 - x^2)) dx, x = r sin t,
    Gauss-Legendre in t, bisection in r"""
    t, w = np.polynomial.legendre.leggauss(400)
    t = t * (math.pi / 2)
    w = w * (math.pi / 2)
    erf = np.vectorize(math.erf)

    def prob(r):
        x = r * np.sin(t)
        half = r * np.cos(t)
        inner = np.ones_like(x) if b == 0.0 else erf(half / (b * math.sqrt(2.0)))
        phi = np.exp(-0.5 * (x / a) ** 2) / (a * math.sqrt(2.0 * math.pi))
        return float(np.sum(w * phi * inner * r * np.cos(t)))

    lo, hi = 1.5 * a, 3.0 * a
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if prob(mid) < 0.95:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def test_hz_pu_close_to_exact_95_radius(built):
    assert exact_radius95(1.0, 0.0) == pytest.approx(1.959964, abs=1e-5)           # one dimension
    assert exact_radius95(1.0, 1.0) == pytest.approx(math.sqrt(-2.0 * math.log(0.05)), rel=1e-9)   # circular: Rayleigh
    for c in np.linspace(0.0, 1.0, 11):
        _, a, b, _, hz, _ = device_math(built, at_origin(0.0025 * c * c, 0.0025, 0.0), 0.0, 0.0)
        assert b / a == pytest.approx(c, abs=1e-15)
        exact = exact_radius95(a, b)
        assert abs(hz - exact) / exact < 3e-3, (c, hz, exact)
