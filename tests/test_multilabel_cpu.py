"""Multi-label plumbing that needs no GPU: the `id b_0 ... b_{C-1}` label-file
reader, the bit-packing convention of the fused BCE loss's label table, the
MULTI_LABEL cfg key, and the two new C-ABI symbols."""
import re

import numpy as np
import pytest

from conftest import ROOT


def _write(path, ids, rows):
    path.write_text("".join(f"{v} {' '.join(str(int(b)) for b in r)}\n" for v, r in zip(ids, rows)))


@pytest.mark.parametrize("C", [1, 33, 121])
def test_reader_round_trips_unordered_ids_and_leaves_unlisted_vertices_zero(tmp_path, C):
    from nts import dataloader
    V = 50
    rng = np.random.default_rng(C)
    want = rng.integers(0, 2, (V, C)).astype(np.uint8)
    want[17] = 0  # vertex 17 is not in the file
    ids = np.array([v for v in rng.permutation(V) if v != 17])
    assert not np.array_equal(ids, np.sort(ids))
    _write(tmp_path / "lab", ids, want[ids])
    got = dataloader.read_multilabel_file(tmp_path / "lab", V, C)
    assert got.dtype == np.uint8 and got.shape == (V, C)
    assert np.array_equal(got, want)
    assert want.any() and not got[17].any()


def test_reader_names_the_malformed_line(tmp_path):
    from nts import dataloader
    p = tmp_path / "lab"
    p.write_text("0 1 0 1\n1 0 0\n2 1 1 1\n")  # line 2: two columns instead of three
    with pytest.raises(ValueError, match=r"lab:2: 2 label columns, expected 3"):
        dataloader.read_multilabel_file(p, 3, 3)
    p.write_text("0 1 0 1\n1 0 0 0\n2 1 2 1\n")  # line 3: an entry that is not 0/1
    with pytest.raises(ValueError, match=r"lab:3: label 1 is '2'"):
        dataloader.read_multilabel_file(p, 3, 3)
    p.write_text("0 1 0 1\n1 0 0.0 0\n")
    with pytest.raises(ValueError, match=r"lab:2: label 1 is '0.0'"):
        dataloader.read_multilabel_file(p, 3, 3)
    p.write_text("0 1 0 1\n7 0 0 0\n")  # id outside [0, V)
    with pytest.raises(ValueError, match=r"lab:2: vertex id 7"):
        dataloader.read_multilabel_file(p, 3, 3)
    p.write_text("0 1 0 1 1\n")  # one column too many
    with pytest.raises(ValueError, match=r"lab:1: 4 label columns, expected 3"):
        dataloader.read_multilabel_file(p, 3, 3)


@pytest.mark.parametrize("C", [1, 31, 32, 33, 100, 128])
def test_bit_packing_convention(C):
    """label c of a vertex is bit c & 31 of word c >> 5 of its row"""
    from nts import dataloader
    rng = np.random.default_rng(100 + C)
    lab = rng.integers(0, 2, (23, C)).astype(np.uint8)
    lab[0] = 1  # every bit, bit 31 of a word included
    bits = dataloader.pack_label_bits(lab)
    wpr = (C + 31) // 32
    assert bits.dtype == np.uint32 and bits.shape == (23, wpr)
    want = np.zeros((23, wpr), np.uint32)
    for v in range(23):
        for c in range(C):
            if lab[v, c]:
                want[v, c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    assert np.array_equal(bits, want)
    back = (bits[:, np.arange(C) >> 5] >> (np.arange(C, dtype=np.uint32) & 31)) & 1
    assert np.array_equal(back.astype(np.uint8), lab)


def test_multi_label_cfg_key_parses(tmp_path, golden):
    from nts import dataloader
    text = (golden / "cora" / "gcn_cora_sample.cfg").read_text()
    (tmp_path / "plain.cfg").write_text(text)
    (tmp_path / "ml.cfg").write_text(text + "MULTI_LABEL:1\n")
    assert dataloader.InputInfo.from_cfg(tmp_path / "plain.cfg").multi_label == 0
    info = dataloader.InputInfo.from_cfg(tmp_path / "ml.cfg")
    assert info.multi_label == 1 and "MULTI_LABEL" not in info.extra


def test_header_and_bindings_list_the_bce_symbols_at_abi_11():
    from nts import _abi
    text = (ROOT / "include" / "nts_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in ("nts_hip_linear_bce_fwd", "nts_hip_linear_bce_train"):
        assert re.search(rf"\bint {sym}\s*\(", code), sym
        assert sym in _abi.EXPORTED
    assert re.search(r"#define\s+NTS_HIP_ABI_VERSION\s+11\b", text)
    assert _abi.ABI_VERSION == 11
    lib = _abi.lib()
    assert lib.nts_hip_abi_version() == 11
    assert lib.nts_hip_linear_bce_fwd.argtypes is not None
    assert len(lib.nts_hip_linear_bce_fwd.argtypes) == 12
    assert len(lib.nts_hip_linear_bce_train.argtypes) == 14
