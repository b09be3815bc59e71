"""Positional and relative uncertainty on the device (dnagpu_block_station_uncertainty / _pair_uncertainty through the dna_adjust facade
and the C-ABI) against numpy applied to the downloaded rigorous variance matrices, and against the precisions of the adjusted GNSS
baselines the statistics already compute."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from dynadjust_amd import _lib, adjust
from dynadjust_amd.device import pack_lower, unpack_lower
from tests import dnaformats as F

pytestmark = pytest.mark.gpu

SP1 = (1.960790, 0.004071, 0.114276, 0.371625)
GRS80_A, GRS80_INV_F = 6378137.0, 298.257222101


def cart_to_geo(x, y, z):
    """geodesy::CartToGeo (dynadjust_amd/csrc/host/geodesy.hpp), the same arithmetic"""
    f = 1.0 / GRS80_INV_F
    a = GRS80_A
    b = a * (1.0 - f)
    p2 = x * x + y * y
    p = math.sqrt(p2)
    a2, b2, z2 = a * a, b * b, z * z
    a2z2, b2p2 = a2 * z2, b2 * p2
    A = a2z2 + b2p2
    m = (a * b * math.sqrt(A) * A - a2 * b2 * A) / (2.0 * (a2 * a2z2 + b2 * b2p2))
    for _ in range(5):
        tm = 2.0 * m
        am, bm = a2 + tm, b2 + tm
        fv = a2 * p2 / (am * am) + b2 * z2 / (bm * bm) - 1.0
        if abs(fv) < 1e-12:
            break
        df = -4.0 * (a2 * p2 / (am * am * am) + b2 * z2 / (bm * bm * bm))
        m -= fv / df
    tm = 2.0 * m
    pE, zE = a2 * p / (a2 + tm), b2 * z / (b2 + tm)
    lat = math.atan(a2 * zE / (b2 * pE))
    lon = math.atan(y / x)
    if x < 0.0 and y > 0.0:
        lon += math.pi
    elif x < 0.0 and y < 0.0:
        lon = -(math.pi - lon)
    return lat, lon


def rotation(lat, lon):
    sl, cl, so, co = math.sin(lat), math.cos(lat), math.sin(lon), math.cos(lon)
    return np.array([[-so, -sl * co, cl * co], [co, -sl * so, cl * so], [0.0, cl, sl]])


def expected_record(D, lat, lon):
    """numpy restatement of uncertainty.h for a 3x3 cartesian covariance"""
    R = rotation(lat, lon)
    Q = R.T @ D @ R
    w, v = np.linalg.eigh(Q[:2, :2])
    a, b = math.sqrt(max(w[1], 0.0)), math.sqrt(max(w[0], 0.0))
    c = b / a if a > 0 else 0.0
    return dict(enu=Q[np.triu_indices(3)], semi_major=a, semi_minor=b, azimuth=math.atan2(v[0, 1], v[1, 1]) % math.pi,
                hz_pu=a * (SP1[0] + SP1[1] * c + SP1[2] * c * c + SP1[3] * c ** 3), vt_pu=1.96 * math.sqrt(max(Q[2, 2], 0.0)))


def check_record(rec, exp, rel=1e-12):
    scale = max(np.abs(exp["enu"]).max(), 1e-300)
    assert np.abs(rec["enu"] - exp["enu"]).max() <= rel * scale
    a = exp["semi_major"]
    for f in ("semi_major", "semi_minor", "hz_pu"):
        assert abs(rec[f] - exp[f]) <= rel * a + 1e-9 * math.sqrt(rel * scale), f    # (b near 0: sqrt of a tiny difference)
    # (the up variance of a held station can be 1e-6 of the horizontal ones: its rounding is relative to the record's scale)
    assert abs((rec["vt_pu"] / 1.96) ** 2 - (exp["vt_pu"] / 1.96) ** 2) <= rel * scale
    if a - exp["semi_minor"] > 1e-4 * a:
        d = abs(rec["azimuth"] - exp["azimuth"]) % math.pi
        assert min(d, math.pi - d) < 1e-8
    assert 0.0 <= rec["azimuth"] < math.pi


class Blocks:
    """the downloaded rigorous results of every block"""

    def __init__(self, a):
        self.stations = [a.block_stations(b) for b in range(a.blockCount())]
        self.xyz = [a.block_estimates(b).reshape(-1, 3) for b in range(a.blockCount())]
        self.V = [unpack_lower(a.block_variances_packed(b), 3 * len(s)) for b, s in enumerate(self.stations)]

    def local(self, b, s):
        l = int(np.searchsorted(self.stations[b], s))
        assert self.stations[b][l] == s
        return l

    def frame(self, b, l):
        return cart_to_geo(*self.xyz[b][l])


def check_positional(a, blk):
    pu = a.GetPositionalUncertainty()
    in_some = set(int(s) for st in blk.stations for s in st)
    for s, rec in enumerate(pu):
        if s not in in_some:
            assert rec["block"] == -1 and not rec["enu"].any()
            continue
        b = int(rec["block"])
        assert b >= 0 and s in set(int(x) for x in blk.stations[b])
        l = blk.local(b, s)
        C3 = blk.V[b][3 * l:3 * l + 3, 3 * l:3 * l + 3]
        lat, lon = blk.frame(b, l)
        check_record(rec, expected_record(C3, lat, lon))
        # the standard deviations e, n, up of DynAdjustPrinter::StationResults
        R = rotation(lat, lon)
        sd2 = np.array([sum(R[i, k] * C3[i, j] * R[j, k] for i in range(3) for j in range(3)) for k in range(3)])
        assert np.abs(rec["enu"][[0, 3, 5]] - sd2).max() <= 1e-12 * np.abs(rec["enu"]).max()
    return pu


def pair_cov(V, li, lj):
    Cii, Cjj = V[3 * li:3 * li + 3, 3 * li:3 * li + 3], V[3 * lj:3 * lj + 3, 3 * lj:3 * lj + 3]
    Cij = V[3 * li:3 * li + 3, 3 * lj:3 * lj + 3]
    return Cii + Cjj - Cij - Cij.T


def check_relative(a, blk):
    ru = a.GetRelativeUncertainty()
    assert len(ru) > 0
    for rec in ru:
        b = int(rec["block"])
        assert b >= 0                              # every measured pair lies in the block of its measurement
        i, j = int(rec["stn1"]), int(rec["stn2"])
        assert b == min(k for k, st in enumerate(blk.stations) if i in st and j in st)
        li, lj = blk.local(b, i), blk.local(b, j)
        lat, lon = blk.frame(b, li)
        check_record(rec, expected_record(pair_cov(blk.V[b], li, lj), lat, lon))
    return ru


def gnss_vectors(recs, cml):
    """(first station, second station, type) of every GNSS vector of a block in CML order (dna_adjust::StatisticsBlock's order)"""
    out = []
    for m in cml:
        r = recs[m]
        t = r["measType"].decode()
        if r["ignore"] or r["measStart"] != 0 or t not in "GXY":
            continue
        k = 1 if t == "G" else int(r["vectorCount1"])
        q = m
        for _ in range(k):
            out.append((int(recs[q]["station1"]), int(recs[q]["station2"]), t))
            q += 3 + (0 if t == "G" else 3 * int(recs[q]["vectorCount2"]))
    return out


def simultaneous_cml(recs):
    """BuildSimultaneousLists: the first record of every measurement, the first vector of a cluster for X / Y"""
    cml, cluster = [], None
    for m, r in enumerate(recs):
        if r["ignore"] or r["measStart"] != 0:
            continue
        t = r["measType"].decode()
        if t == "D" and r["vectorCount1"] < 1:
            continue
        if t in "XY":
            if cluster == int(r["clusterID"]):
                continue
            cluster = int(r["clusterID"])
        cml.append(m)
    return cml


def check_gnss_baselines(a, ru, cmls):
    """cartesian D of every G baseline (R Q R^T from the pair's record) against the adjusted-baseline precision of the statistics"""
    recs = np.frombuffer(a.measurement_records().tobytes(), dtype=F.MEASUREMENT_DT)
    by_pair = {(int(r["stn1"]), int(r["stn2"])): r for r in ru}
    checked = 0
    for b, cml in enumerate(cmls):
        prec = a.block_prec_adj_msrs(b).reshape(-1, 6)
        vec = gnss_vectors(recs, cml)
        assert len(vec) == len(prec)
        for v, (s1, s2, t) in enumerate(vec):
            if t != "G" or (s1, s2) not in by_pair:
                continue
            rec = by_pair[(s1, s2)]
            bb = int(rec["block"])
            st = a.block_stations(bb)
            l1 = int(np.searchsorted(st, s1))
            lat, lon = cart_to_geo(*a.block_estimates(bb).reshape(-1, 3)[l1])
            R = rotation(lat, lon)
            Q = np.zeros((3, 3))
            Q[np.triu_indices(3)] = rec["enu"]
            Q = Q + np.triu(Q, 1).T
            D = (R @ Q @ R.T)[np.triu_indices(3)]
            assert np.abs(D - prec[v]).max() <= 1e-10 * np.abs(prec[v]).max()
            checked += 1
    return checked


def run(folder, name, phased, **kw):
    p = adjust.ProjectSettings(name, folder, adjust_mode=adjust.PhasedMode if phased else adjust.SimultaneousMode, **kw)
    a = adjust.DnaAdjust()
    a.PrepareAdjustment(p)
    assert a.AdjustNetwork() == adjust.ADJUST_SUCCESS
    return a


def statistics_snapshot(a):
    a.GenerateStatistics()
    return (a.GetChiSquared(), a.GetSigmaZero(), a.GetPotentialOutlierCount(), a.measurement_records().tobytes(),
            [a.block_prec_adj_msrs(b).tobytes() for b in range(a.blockCount())])


@pytest.mark.parametrize("phased,stage", [(False, False), (True, False), (True, True)])
def test_tiny_network(built, golden_dir, phased, stage):
    a = run(golden_dir, "tiny_net", phased, stage=stage)
    before = statistics_snapshot(a)
    blk = Blocks(a)
    check_positional(a, blk)
    ru = check_relative(a, blk)
    recs = F.read_bms(os.path.join(golden_dir, "tiny_net.bms"))
    cmls = F.read_seg(os.path.join(golden_dir, "tiny_net.seg"))[2] if phased else [simultaneous_cml(recs)]
    assert check_gnss_baselines(a, ru, cmls) > 0
    # a pair whose stations share no block (phased) is reported, not raised; a pair of one station is zero
    n = int(max(s.max() for s in blk.stations)) + 1
    pairs = [(0, 0)]
    if phased and a.blockCount() > 1:
        far = [(i, j) for i in blk.stations[0] for j in blk.stations[-1] if not any(i in s and j in s for s in blk.stations)]
        assert far
        pairs.append(far[0])
    pairs.append((n + 5, 0))                       # a station that does not exist
    r = a.GetRelativeUncertainty(np.array(pairs, dtype=np.uint32))
    assert r["block"][0] >= 0 and not r["enu"][0].any() and r["hz_pu"][0] == 0.0
    for k in range(1, len(pairs)):
        assert r["block"][k] == -1 and not r["enu"][k].any()
    # the getters leave the statistics as they were, bit for bit
    assert statistics_snapshot(a) == before
    a.close()


def test_gnss_sample_simultaneous(built, golden_dir, tmp_path):
    from tests.dnatext import build_gnss_sample_with_the_product_importer
    base = str(tmp_path / "gnss")
    build_gnss_sample_with_the_product_importer(golden_dir, base)
    a = run(str(tmp_path), "gnss", False)
    a.GenerateStatistics()
    blk = Blocks(a)
    pu = check_positional(a, blk)
    assert (pu["block"] == 0).sum() == len(blk.stations[0])
    ru = check_relative(a, blk)
    recs = np.frombuffer(a.measurement_records().tobytes(), dtype=F.MEASUREMENT_DT)
    assert check_gnss_baselines(a, ru, [simultaneous_cml(recs)]) > 0
    a.close()


def test_urban_sample_phased(built, golden_dir, tmp_path):
    from tests import urban_net as U
    U.build_urban_sample(golden_dir, str(tmp_path / "urban"), blocks=2)
    a = run(str(tmp_path), "urban", True)
    a.GenerateStatistics()
    blk = Blocks(a)
    check_positional(a, blk)
    ru = check_relative(a, blk)
    # terrestrial pairs as well as GNSS ones: more pairs than GNSS vectors
    recs = np.frombuffer(a.measurement_records().tobytes(), dtype=F.MEASUREMENT_DT)
    assert len(ru) > sum(1 for r in recs if not r["ignore"] and r["measStart"] == 0 and r["measType"] in (b"G", b"X"))
    a.close()


def test_in_process_devices_match_one_device(built, golden_dir):
    one = run(golden_dir, "tiny_net", True)
    two = run(golden_dir, "tiny_net", True, devices=[0, 0], dist_transport="local")
    p1, p2 = one.GetPositionalUncertainty(), two.GetPositionalUncertainty()
    assert np.array_equal(p1["block"], p2["block"])
    for f in ("semi_major", "semi_minor", "hz_pu", "vt_pu"):
        assert np.allclose(p1[f], p2[f], rtol=1e-12, atol=0)
    assert np.allclose(p1["enu"], p2["enu"], rtol=1e-12, atol=1e-12 * np.abs(p1["enu"]).max())
    r1, r2 = one.GetRelativeUncertainty(), two.GetRelativeUncertainty()
    assert np.array_equal(r1[["stn1", "stn2", "block"]], r2[["stn1", "stn2", "block"]])
    assert np.allclose(r1["hz_pu"], r2["hz_pu"], rtol=1e-12, atol=0)
    assert np.allclose(r1["enu"], r2["enu"], rtol=1e-12, atol=1e-12 * np.abs(r1["enu"]).max())
    one.close()
    two.close()


def test_printer_tables_are_opt_in(built, golden_dir, tmp_path):
    texts = {}
    for tag, on in (("off", False), ("on", True)):
        out = tmp_path / tag
        out.mkdir()
        a = run(golden_dir, "tiny_net", True, output_folder=str(out), output_pos_uncertainty=on, output_rel_uncertainty=on)
        a.GenerateStatistics()
        a.PrintPositionalUncertainty()
        texts[tag] = open(out / "tiny_net.phased.apu", "rb").read()
        if on:
            n_pu = int((a.GetPositionalUncertainty()["block"] >= 0).sum())
            n_ru = int((a.GetRelativeUncertainty()["block"] >= 0).sum())
        a.close()
    off, on = texts["off"], texts["on"]
    # with the flags off the report is the cartesian table alone; the flags append to it and change nothing before
    assert on.startswith(off) and len(on) > len(off)
    extra = on[len(off):].decode().split("\n")
    assert "Positional Uncertainty" in extra[1] and "Relative Uncertainty" in on[len(off):].decode()
    rows = [l for l in extra if l and not l.startswith(("Positional", "Relative", "Station"))]
    assert len(rows) == n_pu + n_ru


def test_device_entries_check_indices(built, gpu_ctx):
    lib, ctx = gpu_ctx.lib, gpu_ctx
    ns = 5
    rng = np.random.default_rng(7)
    M = rng.normal(size=(3 * ns, 3 * ns)) * 0.01
    S = M @ M.T + np.eye(3 * ns) * 1e-6
    blk = 4242
    ctx.block_create(blk, ns, 0)
    m = ctx.matrix(3 * ns)
    try:
        m.upload_packed(pack_lower(S), 3 * ns)
        out = (_lib.DnaGpuUncertainty * 4)()
        ll = np.array([0.3, 2.1, -0.6, 0.4, 1.2, -2.9, 0.0, 0.0])
        idx = np.array([0, 4, 2, 1], dtype=np.uint32)
        p_ll = ll.ctypes.data_as(C.POINTER(C.c_double))
        assert lib.dnagpu_block_station_uncertainty(ctx.h, 0, blk, m.h, idx.ctypes.data_as(C.POINTER(C.c_uint32)), p_ll, 4, out) == 0
        for k, s in enumerate(idx):
            rec = np.frombuffer(out, dtype=np.float64).reshape(4, 11)[k]
            exp = expected_record(S[3 * s:3 * s + 3, 3 * s:3 * s + 3], ll[2 * k], ll[2 * k + 1])
            assert np.abs(rec[:6] - exp["enu"]).max() <= 1e-12 * np.abs(exp["enu"]).max()
        pairs = np.array([0, 4, 3, 1, 2, 2], dtype=np.uint32)
        assert lib.dnagpu_block_pair_uncertainty(ctx.h, 0, blk, m.h, pairs.ctypes.data_as(C.POINTER(C.c_uint32)), p_ll, 3, out) == 0
        recs = np.frombuffer(out, dtype=np.float64).reshape(4, 11)
        for k in range(3):
            i, j = int(pairs[2 * k]), int(pairs[2 * k + 1])
            exp = expected_record(pair_cov(S, i, j), ll[2 * k], ll[2 * k + 1])
            assert np.abs(recs[k, :6] - exp["enu"]).max() <= 1e-12 * max(np.abs(exp["enu"]).max(), 1e-300)
        assert not recs[2].any()                    # i == j
        # out-of-range indices (and an unknown block) are refused before anything runs on the device
        bad = np.array([0, ns], dtype=np.uint32)
        assert lib.dnagpu_block_station_uncertainty(ctx.h, 0, blk, m.h, bad.ctypes.data_as(C.POINTER(C.c_uint32)), p_ll, 2, out) == -1
        bad = np.array([ns + 100, 0], dtype=np.uint32)
        assert lib.dnagpu_block_pair_uncertainty(ctx.h, 0, blk, m.h, bad.ctypes.data_as(C.POINTER(C.c_uint32)), p_ll, 1, out) == -1
        assert lib.dnagpu_block_station_uncertainty(ctx.h, 0, blk + 1, m.h, idx.ctypes.data_as(C.POINTER(C.c_uint32)), p_ll, 1, out) == -1
        # ... and the context still works
        assert lib.dnagpu_block_station_uncertainty(ctx.h, 0, blk, m.h, idx.ctypes.data_as(C.POINTER(C.c_uint32)), p_ll, 4, out) == 0
        gpu_ctx.sync()
    finally:
        m.close()
        ctx.block_destroy(blk)
