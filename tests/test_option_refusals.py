"""Which refusal the driver's constructor reports when several apply.

tests/test_root_driver.py and tests/test_max_driver.py hold the full text of
every (option, conflict) refusal, one construction each.  This file pins the
order, which a caller sees as "the message I get first": root_weight's
refusals come before aggregator = max's, each option reports its conflicts in
one fixed order, and an aggregator outside {0, 1} is refused between the two.
Every construction fails before the driver touches the device arrays, so the
graph is a toy.
"""
import pytest
import torch

from test_max_driver import REFUSALS as MAX_REFUSALS
from test_root_driver import REFUSALS as ROOT_REFUSALS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAYERS, FANOUT, BATCH = [8, 4, 2], [2, 2], 4
V = 16

# the conflicts both options refuse, in the order the constructor reports them
SHARED = [
    ("gat", dict(gat=True)),
    ("pd_cache", dict(pd_cache=True)),
    ("sample_gpu", dict(sample_gpu=True, rng_mode=1)),
    ("transform_first", dict(transform_first=1)),
    ("pair_table", dict(pair_table=1)),
    ("cache_rate", dict(cache_rate=0.5)),
    ("fused_gather", dict(fused_gather=False)),
    ("deterministic_backward", dict(deterministic_backward=False)),
]


@pytest.fixture(scope="module")
def build():
    from nts import host
    E = host.ext()
    src = torch.arange(V, dtype=torch.int32, device=DEV)
    G = E.FullyRepGraph.from_edges(src, (src + 1) % V, V)
    feat = torch.zeros(V, LAYERS[0], device=DEV)
    labels = torch.zeros(V, dtype=torch.int64, device=DEV)
    train = torch.arange(V, dtype=torch.int32)

    def refusal(cfg_edit=None, **kw):
        cfg = host.gcn_config(LAYERS, FANOUT, BATCH, **kw)
        if cfg_edit:
            cfg_edit(cfg)
        with pytest.raises(RuntimeError) as ei:
            E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, cfg)
        return str(ei.value).splitlines()[0]
    return refusal


@pytest.mark.parametrize("name,kw", SHARED, ids=[n for n, _ in SHARED])
def test_root_weight_is_reported_before_max(build, name, kw):
    assert build(root_weight=True, aggregator="max", **kw) == ROOT_REFUSALS[name]


@pytest.mark.parametrize("first", range(len(SHARED)), ids=[n for n, _ in SHARED])
@pytest.mark.parametrize("option,texts", [(dict(root_weight=True), ROOT_REFUSALS),
                                          (dict(aggregator="max"), MAX_REFUSALS)],
                         ids=["root_weight", "max"])
def test_conflicts_are_reported_in_one_order(build, option, texts, first):
    """every conflict from `first` on at once: the first of them is named"""
    kw = dict(up_degree=True)  # max alone refuses it, after the shared ones
    for _, k in SHARED[first:]:
        kw.update(k)
    assert build(**option, **kw) == texts[SHARED[first][0]]


def test_up_degree_is_reported_after_the_shared_conflicts(build):
    assert build(aggregator="max", up_degree=True) == MAX_REFUSALS["up_degree"]


def test_unknown_aggregator_is_refused_after_root_weight(build):
    def two(cfg):
        cfg.aggregator = 2
    assert build(two) == "aggregator must be 0 (sum) or 1 (max)"
    assert build(two, root_weight=True, pd_cache=True) == ROOT_REFUSALS["pd_cache"]


def test_a_refused_job_allocates_nothing(build):
    """edge_weighted's refusals are the last of the pass, and the pass runs
    before the streams, the arenas and the sampler's slots are made"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    assert build(edge_weighted=True).startswith(
        "edge_weighted is not supported with a graph without edge_prob")
    assert torch.cuda.max_memory_allocated() == before
