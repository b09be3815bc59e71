"""The drop-in boundary, proven from the reference's side: tests/cpp/wrapper_sequence.cpp is a caller written
against the REFERENCE's dna_adjust interface -- dnaadjustwrapper's statements in dnaadjustwrapper's order (dnaadjustwrapper.cpp:1142-1452,
dnaadjustprogress.cpp:49-330) -- compiled against this repository's class and linked to libdnagpu.so by __graft_entry__.build().

CPU: it was built, links, and on a box without a GPU its catch ladder receives the NetAdjustException of PrepareAdjustment.
GPU: it runs the golden 12-station network and the reference's GNSS sample; what it reads through the reference's getters equals
what the same adjustment gives through the C view; the reduced reports of the GetPrinter() adapter carry the adjusted
coordinates and standard deviations; the -rva.mtx / -pam.mtx files it leaves have the byte layout of matrix_2d's stream
operator (dnamatrix_contiguous.cpp:40-101; tests/test_matrix.cpp:1492 pins the size formula)."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from dynadjust_amd import adjust

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "wrapper_sequence")


def _run_wrapper(folder, name, mode, mt=0, report=0):
    r = subprocess.run([EXE, str(folder), name, mode, str(mt), str(report)], capture_output=True, text=True, timeout=600)
    return r


def test_the_caller_was_built_against_the_class(built):
    assert os.path.exists(EXE), "tests/cpp/wrapper_sequence is missing: python __graft_entry__.py"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr
    out = subprocess.run(["ldd", EXE], capture_output=True, text=True).stdout
    assert "libdnagpu.so" in out


def test_without_a_device_the_wrappers_catch_ladder_gets_the_exception(built, golden_dir, tmp_path):
    from dynadjust_amd import _lib
    if _lib.load().dnagpu_device_count() > 0:
        pytest.skip("a GPU is present: PrepareAdjustment succeeds")
    for ext in ("bst", "bms", "asl", "seg"):
        shutil.copy(os.path.join(golden_dir, "tiny_net." + ext), str(tmp_path / ("tiny_net." + ext)))
    r = _run_wrapper(tmp_path, "tiny_net", "phased")
    assert r.returncode == 1
    assert "no MI355X device available" in r.stderr and "prepare" in r.stderr       # dna_adjust_thread::prepareAdjustment's NetAdjustException branch


def _c_view(folder, name, phased, mt):
    a = adjust.DnaAdjust()
    a.PrepareAdjustment(adjust.ProjectSettings(name, str(folder), adjust_mode=adjust.PhasedMode if phased else adjust.SimultaneousMode, multi_thread=bool(mt)))
    st = a.AdjustNetwork()
    a.GenerateStatistics()
    n = a.lib.dnaadj_station_count(a.h)
    out = {"status": st, "iterations": a.CurrentIteration(), "chi_squared": a.GetChiSquared(), "sigma_zero": a.GetSigmaZero(), "dof": a.GetDegreesOfFreedom(),
           "unknowns": a.GetUnknownsCount(), "measurements": a.GetMeasurementCount(), "outliers": a.GetPotentialOutlierCount(), "blocks": a.blockCount(),
           "xyz": a.adjusted_coordinates(n), "var": [a.block_variances_packed(b) for b in range(a.blockCount())], "stations": [a.block_stations(b) for b in range(a.blockCount())],
           "prec": [a.block_prec_adj_msrs(b) for b in range(a.blockCount())], "max_correction": a.GetMaxCorrection()}
    a.close()
    return out


def _read_table(path, title, ncols):
    rows = []
    lines = open(path).read().split("\n")
    i = next(k for k, l in enumerate(lines) if l.startswith(title)) + 2
    while i < len(lines) and lines[i].strip():
        parts = lines[i].split()
        rows.append(parts[-ncols:])
        i += 1
    return np.array(rows, dtype=float)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,mt", [("phased", 0), ("phased", 1), ("simult", 0)])
def test_wrapper_sequence_on_the_golden_network(built, golden_dir, tmp_path, mode, mt):
    for d in ("c", "w"):
        os.makedirs(tmp_path / d)
        for ext in ("bst", "bms", "asl", "seg"):
            shutil.copy(os.path.join(golden_dir, "tiny_net." + ext), str(tmp_path / d / ("tiny_net." + ext)))
    ref = _c_view(tmp_path / "c", "tiny_net", mode == "phased", mt)
    r = _run_wrapper(tmp_path / "w", "tiny_net", mode, mt)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    for k in ("status", "iterations", "dof", "unknowns", "measurements", "outliers", "blocks"):
        assert got[k] == ref[k], k
    assert got["thread_status"] == 0 and got["sinex"] == 0 and got["blas_threads"] == 4
    if mode == "phased":
        assert got["blocks_from_seg"] == ref["blocks"]                  # LoadSegmentationFileParameters before PrepareAdjustment
    for k in ("chi_squared", "sigma_zero", "max_correction"):
        assert abs(got[k] - ref[k]) <= 1e-9 * max(1.0, abs(ref[k])), k
    assert got["progress_lines"] >= got["iterations"]                    # the progress thread saw every iteration's message
    assert "max station corr" in r.stderr
    # the reduced reports of the GetPrinter() adapter
    w = tmp_path / "w"
    tag = "phased" if mode == "phased" else "simult"
    for ext in ("adj", "xyz", "apu", "cor"):
        assert os.path.getsize(w / f"tiny_net.{tag}.{ext}") > 0
    tab = _read_table(w / f"tiny_net.{tag}.xyz", "Adjusted Coordinates", 6)
    assert np.abs(tab[:, :3] - ref["xyz"]).max() < 6e-5                  # printed to 4 decimals
    # standard deviations (e, n, up) of every station from the packed variance matrix of the block in which it is an inner station
    from tests import dnaformats as F
    ISL = F.read_seg(os.path.join(golden_dir, "tiny_net.seg"))[0]
    bst = F.read_bst(os.path.join(golden_dir, "tiny_net.bst"))
    checked = 0
    for b in range(ref["blocks"]):
        st = ref["stations"][b]
        n = 3 * len(st)
        V = np.zeros((n, n))
        idx = 0
        for j in range(n):
            V[j:, j] = ref["var"][b][idx:idx + n - j]
            idx += n - j
        V = V + np.tril(V, -1).T
        inner = set(int(x) for x in ISL[b]) if mode == "phased" else set(st.tolist())
        for l, s in enumerate(st):
            if int(s) not in inner:
                continue
            x, y, z = ref["xyz"][s]
            lon, p = np.arctan2(y, x), np.hypot(x, y)
            lat = np.arctan2(z, p * (1 - 0.00669438002290))
            for _ in range(5):
                N = 6378137.0 / np.sqrt(1 - 0.00669438002290 * np.sin(lat) ** 2)
                lat = np.arctan2(z + 0.00669438002290 * N * np.sin(lat), p)
            R = np.array([[-np.sin(lon), -np.sin(lat) * np.cos(lon), np.cos(lat) * np.cos(lon)],
                          [np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat) * np.sin(lon)], [0.0, np.cos(lat), np.sin(lat)]])
            sd = np.sqrt(np.diag(R.T @ V[3 * l:3 * l + 3, 3 * l:3 * l + 3] @ R))
            assert np.abs(tab[s, 3:] - sd).max() < 6e-5, (b, s)
            checked += 1
    assert checked == len(bst)
    # the variance matrices the wrapper serialised: byte layout of matrix_2d's stream operator, payload = the C view's matrices
    blob = open(w / "tiny_net-rva.mtx", "rb").read()
    off = 0
    for b in range(ref["blocks"]):
        n = 3 * len(ref["stations"][b])
        assert struct.unpack_from("<6I", blob, off) == (1, n, n, n, n, 0)                 # type 1 = symmetric packed lower, rows, cols, mem_rows, mem_cols, pad
        off += 24
        cnt = n * (n + 1) // 2                                                            # tests/test_matrix.cpp:1492: get_size of a packed matrix
        assert np.array_equal(np.frombuffer(blob, dtype="<f8", count=cnt, offset=off), ref["var"][b])
        off += 8 * cnt
        assert struct.unpack_from("<2I", blob, off) == (0, 0)                             # max-value bookkeeping of matrix_2d (row, col)
        off += 8
    assert off == len(blob)
    blob = open(w / "tiny_net-pam.mtx", "rb").read()
    off = 0
    for b in range(ref["blocks"]):
        m = len(ref["prec"][b])
        assert struct.unpack_from("<6I", blob, off) == (0, m, 1, m, 1, 0)                 # type 0 = full column-major
        off += 24
        assert np.array_equal(np.frombuffer(blob, dtype="<f8", count=m, offset=off), ref["prec"][b])
        off += 8 * m + 8
    assert off == len(blob)
    # UpdateBinaryFiles ran: a report-mode run (dnaadjust --report-results) loads the matrices back and prints the same statistics
    r2 = _run_wrapper(w, "tiny_net", mode, mt, report=1)
    assert r2.returncode == 0, r2.stdout + r2.stderr


@pytest.mark.gpu
def test_wrapper_sequence_on_the_reference_gnss_sample(built, golden_dir, tmp_path):
    """sampleData/gnss-network.stn / .msr through the product's importer, then through the wrapper's call sequence: the statistics of the
    reference's published report (gnss.simult.adj.expected: 417 measurements, 129 unknowns, 288 degrees of freedom, sigma zero 1.169,
    10 potential outliers, test passed)"""
    from tests import dnatext as T
    T.build_gnss_sample_with_the_product_importer(golden_dir, str(tmp_path / "gnss"))
    r = _run_wrapper(tmp_path, "gnss", "simult")
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert (got["status"], got["iterations"], got["measurements"], got["unknowns"], got["dof"], got["outliers"], got["test"]) == (0, 2, 417, 129, 288, 10, 0)
    assert abs(got["sigma_zero"] - 1.169) < 6e-4 and abs(got["chi_squared"] - 336.64) < 0.2
    assert abs(got["lower"] - 0.843) < 6e-4 and abs(got["upper"] - 1.170) < 6e-4
    assert got["suspect_lines"] >= 10                                   # PrintSuspectMeasurementSummary lists them
    # (the reference's words, ADJ:7652-7780: no oscillating station here, so one list -- the records beyond the critical value by |N-stat|)
    assert "+ Largest measurement N-statistics (10 total, showing top 10):" in r.stderr and "exceeds critical" in r.stderr
