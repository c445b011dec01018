"""Edge weights as aggregation coefficients (EDGE_WEIGHT_AGG)
without a GPU: the three new C-ABI symbols, the entries' argument checking,
gcn_config, the cfg key, the runner's refusals, and the numpy restatement the
GPU tests compare against (tests/edge_weight_blocks.py) on coefficients of 1."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import edge_weight_blocks as eb
from conftest import GOLDEN, ROOT

CFG = GOLDEN / "cora" / "gcn_cora_sample.cfg"
NEW = ("nts_hip_sample_layer_coef", "nts_hip_spmm_graph_fwd_coef", "nts_hip_spmm_graph_fwd_coef_h")


def test_header_abi_table_and_library_export_the_symbols():
    from nts import _abi
    text = (ROOT / "include" / "nts_hip.h").read_text()
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in _abi.EXPORTED
        assert getattr(_abi.lib(), name).argtypes is not None
    out = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    assert set(NEW) <= set(re.findall(r"\bT (nts_hip_\w+)", out))
    assert re.search(r"^#define NTS_HIP_ABI_VERSION 11\b", text, flags=re.M)
    assert _abi.ABI_VERSION == 11 and _abi.lib().nts_hip_abi_version() == 11


def test_library_refusals_in_argument_checking():
    """Every one fails before any device work (no GPU touched)."""
    from nts import _abi
    lib = _abi.lib()
    dummy = C.create_string_buffer(64)
    p = C.addressof(dummy)
    g = _abi.GraphDev(n_vertices=4, n_edges=4, column_offset=p, row_indices=p, in_degree=p,
                      out_degree=p)

    def out(**kw):
        return _abi.SampCSCDev(v_cap=0, e_cap=0, s_cap=0, destination=p, v_size=p, column_offset=p,
                               row_indices=p, sample_ans=p, edge_dst=p, source=p, sizes=p,
                               edge_weight_forward=p, **kw)

    def call(ep, ec, rng_mode, wt, o):
        return lib.nts_hip_sample_layer_coef(p, C.byref(g), ep, ec, 5, 0, 0, rng_mode, wt, C.byref(o))

    no_wf = out()
    no_wf.edge_weight_forward = None
    cases = [
        ((None, None, _abi.NTS_RNG_PHILOX, _abi.NTS_WEIGHT_SUM, out()), b"edge_coef"),
        ((None, p, _abi.NTS_RNG_MT19937_LEMIRE, _abi.NTS_WEIGHT_SUM, out()), b"MT19937"),
        ((None, p, _abi.NTS_RNG_MT19937_DIV, _abi.NTS_WEIGHT_SUM, out()), b"MT19937"),
        ((None, p, _abi.NTS_RNG_PHILOX, _abi.NTS_WEIGHT_SUM | 0x10, out()), b"UP_DEGREE"),
        ((None, p, _abi.NTS_RNG_PHILOX, _abi.NTS_WEIGHT_SUM, out(omit_map=p)), b"omit_map"),
        ((p, p, _abi.NTS_RNG_PHILOX_SHARED, _abi.NTS_WEIGHT_SUM, out()), b"PHILOX_SHARED"),
        ((None, p, _abi.NTS_RNG_PHILOX, _abi.NTS_WEIGHT_NONE, no_wf), b"edge_weight_forward"),
    ]
    for args, word in cases:
        assert call(*args) == 1 and word in lib.nts_hip_last_error(), word  # NTS_ERR_INVALID
    for name in NEW[1:]:
        rc = getattr(lib, name)(p, C.byref(g), None, 0, 4, _abi.NTS_WEIGHT_SUM, 0, p, 8, 8, p, 8)
        assert rc == 1 and b"edge_coef" in lib.nts_hip_last_error(), name
        rc = getattr(lib, name)(p, C.byref(g), p, 0, 4, _abi.NTS_WEIGHT_MEAN_SAMPLED, 0, p, 8, 8, p, 8)
        assert rc == 1 and b"weight type" in lib.nts_hip_last_error(), name
    assert dummy.raw == b"\0" * 64


def test_gcn_config_round_trips_the_option():
    from nts import _abi, host
    c = host.gcn_config([32, 16, 8], [5, 5], 64, edge_weighted=True)
    assert c.edge_weighted is True and c.rng_mode == _abi.NTS_RNG_PHILOX
    assert c.weighted_sampling is False
    assert host.gcn_config([32, 16, 8], [5, 5], 64).edge_weighted is False
    both = host.gcn_config([32, 16, 8], [5, 5], 64, edge_weighted=True, weighted_sampling=True,
                           weight="none")
    assert both.edge_weighted is True and both.weighted_sampling is True
    shared = host.gcn_config([32, 16, 8], [5, 5], 64, edge_weighted=True, shared_sampling=True)
    assert shared.edge_weighted is True and shared.rng_mode == _abi.NTS_RNG_PHILOX_SHARED


def _info(tmp_path, algo="GCNSAMPLEALLGPU", extra="EDGE_WEIGHT_FILE:w.bin\n"):
    from nts import dataloader
    text = CFG.read_text().replace("ALGORITHM:GCNSAMPLEALLGPU", f"ALGORITHM:{algo}")
    (tmp_path / "job.cfg").write_text(text + "EDGE_WEIGHT_AGG:1\n" + extra)
    return dataloader.InputInfo.from_cfg(tmp_path / "job.cfg")


def test_cfg_key_parses(tmp_path):
    from nts import dataloader
    info = _info(tmp_path)
    assert info.edge_weight_agg == 1 and info.edge_weight_file == "w.bin"
    assert "EDGE_WEIGHT_AGG" not in info.extra
    assert dataloader.InputInfo.from_cfg(CFG).edge_weight_agg == 0


RUN_REFUSALS = [
    ("GCNSAMPLEALLGPU", "", "EDGE_WEIGHT_AGG is not supported without an EDGE_WEIGHT_FILE"),
    ("GATSAMPLEALLGPU", "EDGE_WEIGHT_FILE:w.bin\n", "EDGE_WEIGHT_AGG is not supported with GAT"),
    ("GCNSAMPLEALLGPU", "EDGE_WEIGHT_FILE:w.bin\nAGGREGATOR:max\n",
     "EDGE_WEIGHT_AGG is not supported with AGGREGATOR:max"),
    ("GSSAMPLEALLGPU", "EDGE_WEIGHT_FILE:w.bin\nROOT_WEIGHT:1\n",
     "EDGE_WEIGHT_AGG is not supported with ROOT_WEIGHT:1"),
    ("GCNSAMPLEPDCACHE", "EDGE_WEIGHT_FILE:w.bin\n", "EDGE_WEIGHT_AGG is not supported with the PD-cache"),
    ("GSSAMPLEPDCACHE", "EDGE_WEIGHT_FILE:w.bin\n", "EDGE_WEIGHT_AGG is not supported with the PD-cache"),
    ("GCNSAMPLEGPU", "EDGE_WEIGHT_FILE:w.bin\n", "EDGE_WEIGHT_AGG is not supported with GCNSAMPLEGPU"),
    ("GCNSAMPLESINGLE", "EDGE_WEIGHT_FILE:w.bin\n",
     "EDGE_WEIGHT_AGG is not supported with the mt19937-stream"),
    ("GCNSAMPLEALLGPU", "EDGE_WEIGHT_FILE:w.bin\nUP_DEGREE:1\n",
     "EDGE_WEIGHT_AGG is not supported with UP_DEGREE:1"),
]


@pytest.mark.parametrize("algo,extra,text", RUN_REFUSALS,
                         ids=[t.split("supported ")[1].replace(" ", "-") for _, _, t in RUN_REFUSALS])
def test_run_refuses_the_combination_before_anything_is_loaded(tmp_path, algo, extra, text):
    from nts import run
    info = _info(tmp_path, algo, extra)
    with pytest.raises(SystemExit, match=re.escape(text)):
        run.build_driver(None, info, None, None, None, None, None)
    # run() itself refuses before it touches a device or a data file (none of
    # the cfg's files exist beside this copy)
    with pytest.raises(SystemExit, match=re.escape(text)):
        run.run(tmp_path / "job.cfg", epochs=1, out=lambda s: None)


def test_runner_help_names_the_key():
    from nts import run
    assert "EDGE_WEIGHT_AGG" in run.__doc__


def test_restatement_with_unit_coefficients_is_the_default():
    """a == 1: the weights are the default's bits, and the serial restatement
    is the oracle's aggregation of the same block"""
    from oracle import oracle as orc
    rng = np.random.default_rng(1)
    V = 300
    src, dst = eb.simple_graph(V, 4000, 250, 2)
    col, rows = orc.build_csc(V, src, dst)
    od, idg = orc.degrees(V, src, dst)
    seeds = np.arange(V, dtype=np.uint32)
    for mean in (False, True):
        o = orc.Sampler(col, rows, idg, od, [-1], seed=2000, rng_mode=orc.RNG_PHILOX,
                        order_mode=orc.ORDER_DRAW)
        lay = o.sample(seeds, weight_type=orc.W_MEAN if mean else orc.W_SUM)[0]
        assert lay["e_size"] == rows.size and np.array_equal(lay["sample_ans"], rows)
        q = eb.layer_positions(col, rows, lay)
        assert np.array_equal(q, np.arange(rows.size))
        c = lay["edge_weight_forward"]
        ones = np.ones(rows.size, np.float32)
        w = eb.coef_weights(c, ones, q)
        assert np.array_equal(w.view(np.uint32), c.view(np.uint32))
        x = rng.standard_normal((V, 9)).astype(np.float32)
        ref = orc.fuse_fwd(lay, orc.get_feature(lay["source"], x), od, idg, weight_mean=mean)
        assert np.array_equal(eb.serial_spmm(col, rows, w, x), ref)
        assert np.array_equal(eb.serial_spmm(col, rows, w, x, relu=True), np.maximum(ref, 0))
    # and a coefficient is one fp32 multiply
    a = np.exp2(rng.uniform(-3, 3, rows.size)).astype(np.float32)
    w = eb.coef_weights(c, a, q)
    assert w.dtype == np.float32
    assert np.array_equal(w, (c.astype(np.float64) * a.astype(np.float64)).astype(np.float32))
    assert np.array_equal(eb.coef_weights(np.float32(1), a, q), a)
