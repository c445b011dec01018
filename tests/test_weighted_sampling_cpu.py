"""Edge-weighted neighbour selection (SAMPLE_WEIGHTED) without a
GPU: the numpy restatement the GPU tests compare against
(tests/weighted_blocks.py) against the exact successive-sampling
probabilities, the two new C-ABI symbols, the weight file, the cfg keys, the
runner's refusals and gcn_config."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import weighted_blocks as wb
from conftest import GOLDEN, ROOT

CFG = GOLDEN / "cora" / "gcn_cora_sample.cfg"
SEED = 2000
DRAWS = 40_000


def test_the_word_is_word_p_of_a_stream_of_its_own():
    import shared_blocks as sb
    d, bs = 77, (5 << 32) | 9
    p = np.arange(11, dtype=np.uint32)
    got = wb.philox_word(SEED, d, 1 | wb.LAYER_BIT, bs, p)
    for i in range(11):
        r = sb.philox4x32_10([np.array([i >> 2], np.uint32), np.array([d], np.uint32),
                              np.array([0x40000001], np.uint32), np.array([9], np.uint32)],
                             (SEED, 5))
        assert int(got[i]) == int(r[i & 3][0])
    u = wb.uniforms(SEED, d, 1, bs, p)
    assert ((u > 0) & (u < 1)).all()
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)  # exact in fp32


def _frequencies(weights, n):
    """inclusion counts of every position over DRAWS destinations that share
    one list (destination ids 0 .. DRAWS - 1 key the draws)"""
    w = np.asarray(weights, np.float64)
    d = np.arange(DRAWS, dtype=np.uint32)[:, None]
    p = np.arange(w.size, dtype=np.uint32)[None, :]
    keys = -np.log2(wb.uniforms(SEED, d, 0, 3, p)) / w[None, :]
    assert np.array_equal(keys[5], wb.keys64(SEED, 5, 0, 3, w))
    kept = np.argsort(keys, axis=1, kind="stable")[:, :n]
    assert np.array_equal(np.sort(kept[5]), wb.select_positions(keys[5], n))
    return np.bincount(kept.ravel(), minlength=w.size)


@pytest.mark.parametrize("n", [1, 2, 4])
def test_inclusion_frequencies_are_the_exact_successive_sampling_ones(n):
    w = [1, 2, 3, 4, 5]
    prob = wb.inclusion_probabilities(w, n)
    assert abs(prob.sum() - n) < 1e-12
    if n == 1:
        assert np.allclose(prob, np.array(w) / 15.0)
    counts = _frequencies(w, n)
    sd = np.sqrt(DRAWS * prob * (1 - prob))
    print(f"fanout {n}: counts {counts.tolist()} expected {(DRAWS * prob).round(1).tolist()} "
          f"deviations {((counts - DRAWS * prob) / sd).round(2).tolist()}")
    assert (np.abs(counts - DRAWS * prob) <= 5 * sd).all()


@pytest.mark.parametrize("n", [1, 2, 4])
def test_uniform_weights_give_n_over_deg(n):
    prob = wb.inclusion_probabilities([3.0] * 5, n)
    assert np.allclose(prob, n / 5)
    counts = _frequencies([3.0] * 5, n)
    sd = np.sqrt(DRAWS * (n / 5) * (1 - n / 5))
    assert (np.abs(counts - DRAWS * n / 5) <= 5 * sd).all(), counts


def test_selection_ties_go_to_the_earlier_position_and_short_lists_are_copied():
    assert wb.select_positions(np.array([7, 3, 3, 9, 3], np.uint32), 2).tolist() == [1, 2]
    assert wb.select_positions(np.array([7, 3, 3, 9, 3], np.uint32), 4).tolist() == [0, 1, 2, 4]
    assert wb.select_positions(np.array([2.0, 1.0]), 2).tolist() == [0, 1]
    assert wb.select_positions(np.array([2.0, 1.0]), 5).tolist() == [0, 1]


def test_layer_restatement_on_a_toy_graph():
    from oracle import oracle as orc
    rng = np.random.default_rng(1)
    V, E = 300, 6000
    src = rng.integers(0, V, E).astype(np.uint32)
    dst = rng.integers(0, V, E).astype(np.uint32)
    col, rows = orc.build_csc(V, src, dst)
    od, idg = orc.degrees(V, src, dst)
    ep = wb.csc_edge_prob(dst, rng.uniform(0.5, 4.0, E))
    seeds = np.arange(0, V, 3, dtype=np.uint32)
    lay = wb.weighted_layer64(col, rows, idg, od, ep, seeds, 5, SEED, 0, 0)
    deg = np.diff(col.astype(np.int64))[seeds]
    assert np.array_equal(np.diff(lay["column_offset"].astype(np.int64)), np.minimum(deg, 5))
    assert (np.diff(lay["source"].astype(np.int64)) > 0).all()
    for i in range(seeds.size):  # every kept id is a neighbour, in list order
        a, b = int(lay["column_offset"][i]), int(lay["column_offset"][i + 1])
        nb = rows[int(col[seeds[i]]):int(col[seeds[i] + 1])].tolist()
        it = iter(nb)
        assert all(any(x == y for y in it) for x in lay["sample_ans"][a:b].tolist())
    other = wb.weighted_layer64(col, rows, idg, od, ep, seeds, 5, SEED, 0, 1)
    assert not np.array_equal(other["sample_ans"], lay["sample_ans"])


def test_header_abi_table_and_library_export_the_two_symbols():
    from nts import _abi
    text = (ROOT / "include" / "nts_hip.h").read_text()
    for name in ("nts_hip_sample_layer_weighted", "nts_hip_weighted_keys"):
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in _abi.EXPORTED
        assert getattr(_abi.lib(), name).argtypes is not None
    out = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    assert {"nts_hip_sample_layer_weighted", "nts_hip_weighted_keys"} <= set(
        re.findall(r"\bT (nts_hip_\w+)", out))
    assert re.search(r"^#define NTS_HIP_ABI_VERSION 11\b", text, flags=re.M)
    assert _abi.ABI_VERSION == 11 and _abi.lib().nts_hip_abi_version() == 11


def _dummy_call_args():
    dummy = C.create_string_buffer(64)
    p = C.addressof(dummy)
    from nts import _abi
    g = _abi.GraphDev(n_vertices=4, n_edges=4, column_offset=p, row_indices=p, in_degree=p,
                      out_degree=p)
    o = _abi.SampCSCDev(v_cap=0, e_cap=0, s_cap=0, destination=p, v_size=p, column_offset=p,
                        row_indices=p, sample_ans=p, edge_dst=p, source=p, sizes=p)
    return dummy, p, g, o


def test_library_refuses_null_edge_prob_and_omit_map_in_argument_checking():
    """Both fail before any device work (no GPU touched)."""
    from nts import _abi
    lib = _abi.lib()
    dummy, p, g, o = _dummy_call_args()
    rc = lib.nts_hip_sample_layer_weighted(p, C.byref(g), None, 5, 0, 0, _abi.NTS_WEIGHT_NONE,
                                           C.byref(o))
    assert rc == 1 and b"edge_prob" in lib.nts_hip_last_error()  # NTS_ERR_INVALID
    o.omit_map = p
    rc = lib.nts_hip_sample_layer_weighted(p, C.byref(g), p, 5, 0, 0, _abi.NTS_WEIGHT_NONE,
                                           C.byref(o))
    assert rc == 1 and b"omit_map" in lib.nts_hip_last_error()
    rc = lib.nts_hip_weighted_keys(p, C.byref(g), None, p, 1, 0, 0, p, p)
    assert rc == 1 and b"edge_prob" in lib.nts_hip_last_error()
    assert dummy.raw == b"\0" * 64


def test_weight_file_round_trip_and_wrong_size(tmp_path):
    from nts import dataloader
    w = np.random.default_rng(2).uniform(2.0 ** -60, 4.0, 1000).astype(np.float32)
    w[:3] = (2.0 ** -60, 2.0 ** 60, 1.0)
    dataloader.write_edge_weight_file(tmp_path / "w.bin", w.astype(np.float64))
    assert (tmp_path / "w.bin").stat().st_size == 4000
    assert (tmp_path / "w.bin").read_bytes()[8:12] == b"\x00\x00\x80\x3f"  # little-endian 1.0f
    got = dataloader.read_edge_weights(tmp_path / "w.bin", 1000)
    assert got.dtype == np.float32 and np.array_equal(got, w)
    for n in (999, 1001, 0):
        with pytest.raises(ValueError, match="4000 bytes, expected"):
            dataloader.read_edge_weights(tmp_path / "w.bin", n)
        with pytest.raises(ValueError, match="4000 bytes, expected"):
            dataloader.load_edge_weights_to_device(tmp_path / "w.bin", n, "cpu")


def test_cfg_keys_parse(tmp_path):
    from nts import dataloader
    (tmp_path / "job.cfg").write_text(CFG.read_text() + "EDGE_WEIGHT_FILE:w.bin\nSAMPLE_WEIGHTED:1\n")
    info = dataloader.InputInfo.from_cfg(tmp_path / "job.cfg")
    assert info.edge_weight_file == "w.bin" and info.sample_weighted == 1
    assert "EDGE_WEIGHT_FILE" not in info.extra and "SAMPLE_WEIGHTED" not in info.extra
    info = dataloader.InputInfo.from_cfg(CFG)
    assert info.edge_weight_file == "" and info.sample_weighted == 0


def _info(tmp_path, algo="GCNSAMPLEALLGPU", extra="EDGE_WEIGHT_FILE:w.bin\n"):
    from nts import dataloader
    text = CFG.read_text().replace("ALGORITHM:GCNSAMPLEALLGPU", f"ALGORITHM:{algo}")
    (tmp_path / "job.cfg").write_text(text + "SAMPLE_WEIGHTED:1\n" + extra)
    return dataloader.InputInfo.from_cfg(tmp_path / "job.cfg")


def test_run_refuses_the_key_without_a_weight_file(tmp_path):
    from nts import run
    with pytest.raises(SystemExit, match="SAMPLE_WEIGHTED is not supported without an "
                                         "EDGE_WEIGHT_FILE"):
        run.build_driver(None, _info(tmp_path, extra=""), None, None, None, None, None)


@pytest.mark.parametrize("algo", ["GCNSAMPLESINGLE", "GCNSAMPLEGPU", "GCNSAMPLEPDCACHE",
                                  "GSSAMPLEPDCACHE"])
def test_run_refuses_the_key_for_mt_and_pd_cache_algorithms(tmp_path, algo):
    from nts import run
    assert run.ALGORITHMS[algo][2] == "mt" or run.ALGORITHMS[algo][4] == "pd"
    with pytest.raises(SystemExit, match="SAMPLE_WEIGHTED is not supported with the "
                                         "mt19937-stream or PD-cache algorithms"):
        run.build_driver(None, _info(tmp_path, algo), None, None, None, None, None)


def test_run_refuses_the_key_with_sample_shared(tmp_path):
    from nts import run
    info = _info(tmp_path, extra="EDGE_WEIGHT_FILE:w.bin\nSAMPLE_SHARED:1\n")
    with pytest.raises(SystemExit, match="SAMPLE_WEIGHTED is not supported with SAMPLE_SHARED:1"):
        run.build_driver(None, info, None, None, None, None, None)


def test_runner_help_names_the_two_keys():
    from nts import run
    assert "EDGE_WEIGHT_FILE" in run.__doc__ and "SAMPLE_WEIGHTED" in run.__doc__


def test_gcn_config_sets_the_option_and_refuses_mt_and_shared():
    from nts import _abi, host
    c = host.gcn_config([32, 16, 8], [5, 5], 64, weighted_sampling=True)
    assert c.weighted_sampling is True and c.rng_mode == _abi.NTS_RNG_PHILOX
    assert host.gcn_config([32, 16, 8], [5, 5], 64).weighted_sampling is False
    for mt in (_abi.NTS_RNG_MT19937_LEMIRE, _abi.NTS_RNG_MT19937_DIV):
        with pytest.raises(ValueError, match="weighted_sampling is not supported with an MT19937"):
            host.gcn_config([32, 16, 8], [5, 5], 64, weighted_sampling=True, rng_mode=mt)
    with pytest.raises(ValueError, match="weighted_sampling is not supported with shared_sampling"):
        host.gcn_config([32, 16, 8], [5, 5], 64, weighted_sampling=True, shared_sampling=True)
    with pytest.raises(ValueError, match="weighted_sampling is not supported with shared_sampling"):
        host.gcn_config([32, 16, 8], [5, 5], 64, weighted_sampling=True,
                        rng_mode=_abi.NTS_RNG_PHILOX_SHARED)
