"""The f16 feature table without a device: the cfg key, the config
field, the three declared entry points and their ctypes signatures, the
runner's refusals, and the exactness of the widening the GPU tests' references
rest on."""
import pathlib
import re

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
ENTRIES = ("nts_hip_spmm_csc_fwd_h", "nts_hip_spmm_graph_fwd_h", "nts_hip_gather_rows_h")


def _cfg(tmp_path, golden, algorithm):
    text = (golden / "cora" / "gcn_cora_sample.cfg").read_text()
    text = text.replace("ALGORITHM:GCNSAMPLEALLGPU", f"ALGORITHM:{algorithm}")
    (tmp_path / "f16.cfg").write_text(text + "FEATURE_F16:1\n")
    return tmp_path / "f16.cfg"


def test_cfg_key_parses(tmp_path, golden):
    from nts import dataloader
    assert dataloader.InputInfo.from_cfg(_cfg(tmp_path, golden, "GCNSAMPLEALLGPU")).feature_f16 == 1
    assert dataloader.InputInfo.from_cfg(golden / "cora" / "gcn_cora_sample.cfg").feature_f16 == 0


def test_config_field_defaults_off():
    from nts import host
    assert host.gcn_config([32, 16, 8], [5, 5], 64).feature_f16 is False
    assert host.gcn_config([32, 16, 8], [5, 5], 64, feature_f16=True).feature_f16 is True


def test_header_declares_the_entry_points_and_abi_carries_their_signatures():
    import ctypes as C
    from nts import _abi
    header = (ROOT / "include" / "nts_hip.h").read_text()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _abi.EXPORTED
    assert "#define NTS_HIP_ABI_VERSION 11" in header
    L = _abi.lib()
    P, U32, U64, I = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    want = {
        "nts_hip_spmm_csc_fwd_h": [P, P, P, P, P, U32, P, U64, P, U32, P, U64],
        "nts_hip_spmm_graph_fwd_h": [P, C.POINTER(_abi.GraphDev), U64, U64, I, I, P, U64, U32, P, U64],
        "nts_hip_gather_rows_h": [P, P, U64, P, P, U32, U32, P, U64],
    }
    for name, args in want.items():
        fn = getattr(L, name)
        assert list(fn.argtypes) == args and fn.restype is I, name
    # the fp32 siblings' argument lists, a half table in place of the fp32 one
    for name in ENTRIES:
        assert list(getattr(L, name).argtypes) == list(getattr(L, name[:-2]).argtypes)


@pytest.mark.parametrize("algorithm", ["GATSAMPLEALLGPU", "GCNSAMPLEPDCACHE", "GSSAMPLEPDCACHE"])
def test_gat_and_pd_cache_algorithms_refuse_it(tmp_path, golden, algorithm):
    from nts import dataloader, run
    info = dataloader.InputInfo.from_cfg(_cfg(tmp_path, golden, algorithm))
    with pytest.raises(SystemExit) as ei:
        run.build_driver(None, info, None, None, None, None, None)
    assert str(ei.value) == (f"ALGORITHM {algorithm}: FEATURE_F16 is not supported with GAT or "
                             "PD-cache algorithms (the sum aggregation of GCN / GraphSAGE only)")


def test_numpy_widening_is_exact_on_every_finite_half():
    """float16 -> float32 as the GPU tests' references do it, against the value
    the bits spell out: sign, 5-bit exponent (bias 15), 10-bit fraction, the
    subnormals 2^-24 f.  Every finite pattern; the signs of the zeros too."""
    bits = np.arange(1 << 16, dtype=np.uint32)
    sign = np.where(bits >> 15, -1.0, 1.0)
    e = ((bits >> 10) & 31).astype(np.int64)
    f = (bits & 1023).astype(np.float64)
    finite = e != 31
    assert int(finite.sum()) == 65536 - 2048
    value = np.where(e == 0, np.ldexp(f, -24), np.ldexp(1024.0 + f, e - 25)) * sign
    wide = bits.astype(np.uint16).view(np.float16).astype(np.float32)
    assert np.isfinite(wide[finite]).all() and not np.isfinite(wide[~finite]).any()
    got, ref = wide[finite], value[finite].astype(np.float32)
    assert np.array_equal(ref.astype(np.float64), value[finite])  # every half fits a float
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # and back: the widened value rounds to the half it came from
    assert np.array_equal(got.astype(np.float16).view(np.uint16), bits[finite].astype(np.uint16))
