"""Shared-variate neighbour selection (NTS_RNG_PHILOX_SHARED)
without a GPU: the numpy restatement the GPU tests compare against
(tests/shared_blocks.py) on its own, its statistics, and the option through
gcn_config, the cfg key, the runner and the C ABI's argument check."""
import ctypes as C
import re

import numpy as np
import pytest

import shared_blocks as sb
from conftest import GOLDEN, ROOT
from oracle import oracle as orc

CFG = GOLDEN / "cora" / "gcn_cora_sample.cfg"
SEED = 2000


def test_philox_restatement_matches_the_known_answers_and_the_kernel_tests_reference():
    from test_hip_kernels import _philox4x32_10 as theirs
    for c, k, want in sb.PHILOX_KAT:
        got = sb.philox4x32_10([np.array([x], np.uint32) for x in c], k)
        assert tuple(int(x[0]) for x in got) == want
        ref = theirs([np.array([x], np.uint32) for x in c], k)
        assert tuple(int(x[0]) for x in ref) == want
    rng = np.random.default_rng(0)
    c = [rng.integers(0, 2**32, 500, dtype=np.uint64).astype(np.uint32) for _ in range(4)]
    for a, b in zip(sb.philox4x32_10(c, (123, 456)), theirs(c, (123, 456))):
        assert np.array_equal(a, b)


def test_r_is_word_zero_of_the_stream_with_the_layer_bit():
    s = np.array([0, 1, 77, 2**32 - 1], np.uint32)
    bs = (5 << 32) | 9
    want = sb.philox4x32_10([np.zeros(4, np.uint32), s, np.full(4, 0x80000001, np.uint32),
                             np.full(4, 9, np.uint32)], (SEED, 5))[0]
    assert np.array_equal(sb.shared_r(s, SEED, 1, bs), want)


def _toy(seed=1, V=400, E=12000):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, V, E).astype(np.uint32)
    dst = rng.integers(0, V, E).astype(np.uint32)
    col, rows = orc.build_csc(V, src, dst)
    od, idg = orc.degrees(V, src, dst)
    return V, col, rows, idg, od


def test_counts_order_and_independence_of_the_evaluation_order():
    V, col, rows, idg, od = _toy()
    dst = np.arange(0, V, 3, dtype=np.uint32)
    deg = (col[dst + 1] - col[dst]).astype(np.int64)
    for fan in (1, 10, 30, 31, -1):
        a = sb.shared_layer(col, rows, idg, od, dst, fan, SEED, 0, 4)
        want = deg if fan < 0 else np.minimum(deg, fan)
        assert np.array_equal(np.diff(a["column_offset"].astype(np.int64)), want)
        for i, d in enumerate(dst):
            nb = rows[int(col[d]):int(col[d + 1])]
            pos = sb.select_positions(nb, int(want[i]), SEED, 0, 4)
            assert pos.size == want[i] and (np.diff(pos) > 0).all()
            assert np.array_equal(a["sample_ans"][a["column_offset"][i]:a["column_offset"][i + 1]],
                                  nb[pos])
        order = np.random.default_rng(fan + 7).permutation(dst.size)
        b = sb.shared_layer(col, rows, idg, od, dst, fan, SEED, 0, 4, order=order)
        for k in a:
            assert np.array_equal(a[k], b[k]), k


def test_layer_from_selection_agrees_with_the_oracle_on_a_full_neighbourhood():
    """fanout -1 selects nothing at random: the helper's source / relabel /
    weights / CSR must be the oracle's, for every weight type and merged."""
    V, col, rows, idg, od = _toy(2)
    seeds = np.arange(0, V, 5, dtype=np.uint32)
    for flags in (orc.W_SUM, orc.W_MEAN, orc.W_NONE, orc.W_MEAN_SAMPLED, orc.W_SUM | orc.W_UP_DEGREE,
                  orc.W_SUM | orc.F_MERGE_SRC_DST):
        o = orc.Sampler(col, rows, idg, od, [-1, -1], seed=SEED, rng_mode=orc.RNG_PHILOX,
                        order_mode=orc.ORDER_DRAW)
        ol = o.sample(seeds, 0, flags)
        merge = bool(flags & orc.F_MERGE_SRC_DST)
        hl = sb.shared_sample(col, rows, idg, od, seeds, [-1, -1], SEED, 0, flags & 0x1F, merge)
        for a, b in zip(hl, ol):
            for k in a:
                if k in b and not ((flags & 0xF) == orc.W_NONE and "weight" in k):
                    assert np.array_equal(a[k], b[k]), (flags, k)


def test_same_list_same_set_and_parallel_edges_tie_to_the_earlier_position():
    nb = np.random.default_rng(3).permutation(500)[:60].astype(np.uint32)
    a = sb.select_positions(nb, 10, SEED, 1, 2)
    assert np.array_equal(a, sb.select_positions(nb.copy(), 10, SEED, 1, 2))
    # every source twice: a pair shares r, so it is kept together or the
    # earlier position alone (odd n)
    twice = np.concatenate([nb, nb])
    for n in (1, 7, 10):
        pos = sb.select_positions(twice, n, SEED, 1, 2)
        first, second = set(pos[pos < 60].tolist()), set((pos[pos >= 60] - 60).tolist())
        assert second <= first and len(first) - len(second) == n % 2
    r = sb.shared_r(nb, SEED, 1, 2)
    j = int(np.argmin(r))
    assert sb.select_positions(twice, 1, SEED, 1, 2).tolist() == [j]


def test_layer_batch_seq_and_seed_each_change_the_keys():
    s = np.arange(1000, dtype=np.uint32)
    base = sb.shared_r(s, SEED, 0, 0)
    for other in (sb.shared_r(s, SEED, 1, 0), sb.shared_r(s, SEED, 0, 1),
                  sb.shared_r(s, SEED, 0, 1 << 32), sb.shared_r(s, SEED + 1, 0, 0),
                  sb.shared_r(s, SEED + (1 << 32), 0, 0)):
        assert (other != base).mean() > 0.99


def test_marginal_uniformity_of_one_destination():
    """deg 40, fanout 10, 4,000 batch_seq values: every position's count is
    Binomial(4000, 1/4); 5 sigma = 5 sqrt(750) = 136.9."""
    nb = (np.arange(40, dtype=np.uint32) * 7919 + 13) % 100003
    counts = np.zeros(40, np.int64)
    for bs in range(4000):
        counts[sb.select_positions(nb, 10, SEED, 0, bs)] += 1
    print("marginal counts: min", counts.min(), "max", counts.max())
    assert counts.sum() == 40000
    assert (np.abs(counts - 1000) <= 5 * np.sqrt(750.0)).all(), counts


def test_shared_keys_shrink_the_frontier():
    """chung_lu graph of tests/test_gat_full_driver.py's size, fanouts [10, 5],
    1,024 seeds: the hop-1 frontier under shared keys is strictly smaller than
    under the per-destination draws of the PHILOX mode."""
    from nts import synthetic
    g = synthetic.chung_lu(6000, 180000, 20.0, device="cpu", seed=3)
    V = g.n_vertices
    src, dst = g.src.numpy().view(np.uint32), g.dst.numpy().view(np.uint32)
    col, rows = orc.build_csc(V, src, dst)
    od, idg = orc.degrees(V, src, dst)
    seeds = np.arange(1024, dtype=np.uint32)
    o = orc.Sampler(col, rows, idg, od, [10, 5], seed=SEED, rng_mode=orc.RNG_PHILOX,
                    order_mode=orc.ORDER_DRAW)
    plain = o.sample(seeds)
    shared = sb.shared_sample(col, rows, idg, od, seeds, [10, 5], SEED, 0)
    print("hop-0 sources: philox", plain[0]["src_size"], "shared", shared[0]["src_size"])
    print("hop-1 sources: philox", plain[1]["src_size"], "shared", shared[1]["src_size"])
    assert shared[0]["e_size"] == plain[0]["e_size"]
    assert shared[1]["src_size"] < plain[1]["src_size"]


def test_gcn_config_sets_the_mode_and_refuses_an_mt_stream():
    from nts import _abi, host
    c = host.gcn_config([32, 16, 8], [5, 5], 64, shared_sampling=True)
    assert c.rng_mode == _abi.NTS_RNG_PHILOX_SHARED == 3
    assert host.gcn_config([32, 16, 8], [5, 5], 64).rng_mode == _abi.NTS_RNG_PHILOX
    assert host.gcn_config([32, 16, 8], [5, 5], 64, shared_sampling=False,
                           rng_mode=1).rng_mode == _abi.NTS_RNG_MT19937_LEMIRE
    assert host.gcn_config([32, 16, 8], [5, 5], 64, rng_mode=3).rng_mode == 3
    for mt in (_abi.NTS_RNG_MT19937_LEMIRE, _abi.NTS_RNG_MT19937_DIV):
        with pytest.raises(ValueError, match="shared_sampling is not supported with an MT19937"):
            host.gcn_config([32, 16, 8], [5, 5], 64, shared_sampling=True, rng_mode=mt)


def test_cfg_key_parses(tmp_path):
    from nts import dataloader
    (tmp_path / "job.cfg").write_text(CFG.read_text() + "SAMPLE_SHARED:1\nSEED:7\n")
    info = dataloader.InputInfo.from_cfg(tmp_path / "job.cfg")
    assert info.sample_shared == 1 and info.seed == 7
    assert "SAMPLE_SHARED" not in info.extra and "SEED" not in info.extra
    info = dataloader.InputInfo.from_cfg(CFG)
    assert info.sample_shared == 0 and info.seed == 2000


@pytest.mark.parametrize("algo", ["GCNSAMPLESINGLE", "GCNSAMPLEGPU", "GCNSAMPLEPDCACHE",
                                  "GSSAMPLEPDCACHE"])
def test_run_refuses_the_key_for_mt_and_pd_cache_algorithms(tmp_path, algo):
    from nts import dataloader, run
    assert run.ALGORITHMS[algo][2] == "mt" or run.ALGORITHMS[algo][4] == "pd"
    text = CFG.read_text().replace("ALGORITHM:GCNSAMPLEALLGPU", f"ALGORITHM:{algo}")
    (tmp_path / "job.cfg").write_text(text + "SAMPLE_SHARED:1\n")
    info = dataloader.InputInfo.from_cfg(tmp_path / "job.cfg")
    with pytest.raises(SystemExit, match="SAMPLE_SHARED is not supported"):
        run.build_driver(None, info, None, None, None, None, None)


def test_abi_constant_header_and_version():
    from nts import _abi
    assert _abi.NTS_RNG_PHILOX_SHARED == 3
    text = (ROOT / "include" / "nts_hip.h").read_text()
    assert re.search(r"^#define NTS_RNG_PHILOX_SHARED 3$", text, flags=re.M)
    assert re.search(r"^#define NTS_HIP_ABI_VERSION 11\b", text, flags=re.M)
    assert _abi.ABI_VERSION == 11 and _abi.lib().nts_hip_abi_version() == 11


def test_library_refuses_rng_mode_4_in_argument_checking():
    """Fails before any device work (no GPU touched): the pointers only have to
    be non-NULL to reach the rng_mode check."""
    from nts import _abi
    lib = _abi.lib()
    dummy = C.create_string_buffer(64)
    p = C.addressof(dummy)
    g = _abi.GraphDev(n_vertices=4, n_edges=4, column_offset=p, row_indices=p, in_degree=p,
                      out_degree=p)
    o = _abi.SampCSCDev(v_cap=0, e_cap=0, s_cap=0, destination=p, v_size=p, column_offset=p,
                        row_indices=p, sample_ans=p, edge_dst=p, source=p, sizes=p)
    rc = lib.nts_hip_sample_layer(p, C.byref(g), 5, 0, 0, 4, _abi.NTS_WEIGHT_NONE, C.byref(o))
    assert rc == 1  # NTS_ERR_INVALID
    assert b"rng_mode" in lib.nts_hip_last_error()
    rc = lib.nts_hip_sample_layer(p, C.byref(g), 5, 0, 0, -1, _abi.NTS_WEIGHT_NONE, C.byref(o))
    assert rc == 1 and b"rng_mode" in lib.nts_hip_last_error()
