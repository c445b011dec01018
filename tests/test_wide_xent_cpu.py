"""hip_linear_xent_supported, the predicate the drivers ask before they take
the fused output layer + softmax loss: bound in the host extension, true over
the wide range 64 < C <= 512 (K % 16 == 0, K <= 512) and unchanged at C <= 64.
Needs no GPU."""
import pytest


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


def test_the_predicate_is_bound(E):
    assert callable(E.hip_linear_xent_supported)


@pytest.mark.parametrize("K,C", [(256, 172), (16, 65), (512, 512), (128, 349)])
def test_wide_shapes_are_supported(E, K, C):
    assert E.hip_linear_xent_supported(K, C)
    assert E.hip_linear_xent_supported(K=K, C=C)


@pytest.mark.parametrize("K,C", [(24, 100), (16, 513), (16, 0), (528, 512), (0, 100)])
def test_shapes_outside_the_range_are_not(E, K, C):
    assert not E.hip_linear_xent_supported(K, C)


@pytest.mark.parametrize("K,C", [(128, 41), (16, 64)])
def test_narrow_shapes_are_unchanged(E, K, C):
    assert E.hip_linear_xent_supported(K, C)


def test_the_narrow_lds_bound_is_unchanged(E):
    # W [K x 64], 64 Y rows at pitch K + 4 and 64 dZ rows within 160 KB: K = 272 is the last
    assert E.hip_linear_xent_supported(272, 64) and not E.hip_linear_xent_supported(288, 64)
