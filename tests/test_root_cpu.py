"""GraphSAGE root weight, the parts that need no GPU: the exported symbols, the
ROOT_WEIGHT cfg key, the argument checks of the three entry points and the
config field."""
import ctypes

from conftest import GOLDEN
from nts import dataloader

CFG = GOLDEN / "cora" / "gcn_cora_sample.cfg"
SYMBOLS = ("nts_hip_spmm_csc_fwd_root", "nts_hip_root_inverse_map", "nts_hip_spmm_csr_bwd_root")


def test_symbols_are_declared_and_exported():
    from nts import _abi
    lib = _abi.lib()
    for name in SYMBOLS:
        assert name in _abi.EXPORTED
        assert getattr(lib, name).argtypes is not None
    assert lib.nts_hip_abi_version() == 11


def test_root_weight_key_parses_and_defaults_to_off(tmp_path):
    assert dataloader.InputInfo.from_cfg(CFG).root_weight == 0
    (tmp_path / "job.cfg").write_text(CFG.read_text() + "ROOT_WEIGHT:1\n")
    info = dataloader.InputInfo.from_cfg(tmp_path / "job.cfg")
    assert info.root_weight == 1
    assert info.layers == [1433, 256, 7]  # the rest of the job is unchanged


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from nts import _abi
    lib = _abi.lib()
    buf = (ctypes.c_uint32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # any non-NULL address: nothing is launched

    def invalid(rc, what):
        assert rc == 1  # NTS_ERR_INVALID
        assert b"invalid argument" in lib.nts_hip_last_error()
        assert what in lib.nts_hip_last_error()

    fwd, inv, bwd = (getattr(lib, s) for s in SYMBOLS)
    # (ctx, co, ri, w, v, v_cap, x, ldx, map, self, F, ycat, ld_ycat)
    invalid(fwd(None, p, p, p, p, 4, p, 8, None, p, 8, p, 16), b"NULL")
    invalid(fwd(p, p, p, p, p, 4, p, 8, None, None, 8, p, 16), b"NULL")
    invalid(fwd(p, p, p, p, p, 4, p, 8, None, p, 8, None, 16), b"NULL")
    invalid(fwd(p, p, p, p, p, 4, p, 8, None, p, 8, p, 15), b"ld_ycat")
    invalid(fwd(p, p, p, p, p, 4, p, 8, None, p, 0, p, 16), b"feature_size")
    # (ctx, dst_local_id, v, v_cap, s, s_cap, src_dst)
    invalid(inv(p, None, p, 4, p, 4, p), b"NULL")
    invalid(inv(p, p, p, 4, p, 4, None), b"NULL")
    # (ctx, ro, ci, wb, s, s_cap, g, ld_g, src_dst, x_act, ld_act, scale, F, g_in, ld_gin)
    invalid(bwd(p, p, p, p, p, 4, p, 16, None, None, 0, 1.0, 8, p, 8), b"NULL")
    invalid(bwd(p, p, p, p, p, 4, None, 16, p, None, 0, 1.0, 8, p, 8), b"NULL")
    invalid(bwd(p, p, p, p, p, 4, p, 15, p, None, 0, 1.0, 8, p, 8), b"ld_ycat")
    invalid(bwd(p, p, p, p, p, 4, p, 16, p, None, 0, 1.0, 0, p, 8), b"feature_size")
    invalid(bwd(p, p, p, p, p, 4, p, 16, p, p, 7, 1.0, 8, p, 8), b"leading dimension")


def test_gcn_config_sets_the_field():
    from nts import host
    assert host.gcn_config([32, 16, 8], [5, 5], 64).root_weight is False
    assert host.gcn_config([32, 16, 8], [5, 5], 64, root_weight=True).root_weight is True
