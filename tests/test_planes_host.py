"""walker_set_create's layout work (lisp-mcmc_amd/walker.py: planes_layout, data_separated): what
a list of datasets, a plist or a list of plists and the five shapes of :data-error become before
any engine exists.  Needs no device."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def W():
    from lisp_mcmc_amd import walker
    return walker


@pytest.fixture(scope="module")
def capi():
    from lisp_mcmc_amd import capi
    return capi


C, N = 5, 7


def datasets(seed=0):
    rng = np.random.default_rng(seed)
    x = np.linspace(2.0, 3.0, N)
    return [[x.copy(), rng.normal(size=N)] for _ in range(C)]


PARAMS = [":b", 1.0, ":m", 2.0]


def test_the_five_data_error_shapes_map_to_the_four_kinds(W, capi):
    ds = datasets()
    rng = np.random.default_rng(1)
    per_walker = list(rng.uniform(0.1, 0.2, C))
    per_point = list(rng.uniform(0.1, 0.2, N))
    per_both = [list(rng.uniform(0.1, 0.2, N)) for _ in range(C)]
    lay = W.planes_layout(ds, PARAMS, None)
    assert lay["sigma_kind"] == capi.SIGMA_NONE and lay["sigma"] is None
    assert np.array_equal(lay["sigma_rows"], np.ones((C, N)))
    lay = W.planes_layout(ds, PARAMS, 0.25)
    assert lay["sigma_kind"] == capi.SIGMA_PER_CHAIN and np.array_equal(lay["sigma"], np.full(C, 0.25))
    assert np.array_equal(lay["sigma_rows"], np.full((C, N), 0.25))
    lay = W.planes_layout(ds, PARAMS, per_walker)
    assert lay["sigma_kind"] == capi.SIGMA_PER_CHAIN and np.array_equal(lay["sigma"], per_walker)
    assert all(np.array_equal(lay["sigma_rows"][c], np.full(N, per_walker[c])) for c in range(C))
    lay = W.planes_layout(ds, PARAMS, per_point)
    assert lay["sigma_kind"] == capi.SIGMA_SHARED and np.array_equal(lay["sigma"], per_point)
    assert all(np.array_equal(lay["sigma_rows"][c], per_point) for c in range(C))
    lay = W.planes_layout(ds, PARAMS, per_both)
    assert lay["sigma_kind"] == capi.SIGMA_PER_POINT and lay["sigma"].shape == (C, N)
    assert np.array_equal(lay["sigma"], per_both) and np.array_equal(lay["sigma_rows"], per_both)
    assert lay["sigma"].flags["C_CONTIGUOUS"]
    for bad in ([0.1, 0.2], [[0.1] * N] * (C - 1), [[0.1] * (N - 1)] * C):
        with pytest.raises(ValueError, match="data_error"):
            W.planes_layout(ds, PARAMS, bad)


def test_as_many_points_as_walkers_is_read_per_walker(W, capi):
    ds = [[np.arange(3.0), np.zeros(3)] for _ in range(3)]
    lay = W.planes_layout(ds, PARAMS, [0.1, 0.2, 0.3])
    assert lay["sigma_kind"] == capi.SIGMA_PER_CHAIN
    assert np.array_equal(lay["sigma_rows"][1], [0.2, 0.2, 0.2])


def test_x_and_y_planes(W):
    ds = datasets(3)
    lay = W.planes_layout(ds, PARAMS)
    assert lay["x"].dtype == np.float64 and np.array_equal(lay["x"], ds[0][0])
    assert lay["y"].shape == (C, N) and lay["y"].flags["C_CONTIGUOUS"]
    for c in range(C):
        assert np.array_equal(lay["y"][c], ds[c][1])


def test_one_plist_or_one_per_walker(W):
    ds = datasets()
    lay = W.planes_layout(ds, PARAMS)
    assert lay["keys"] == ["b", "m"] and np.array_equal(lay["theta0"], np.tile([1.0, 2.0], (C, 1)))
    lay = W.planes_layout(ds, {"b": 1.0, "m": 2.0})
    assert lay["keys"] == ["b", "m"] and lay["theta0"].shape == (C, 2)
    each = [[":b", 1.0 + c, ":m", 2.0 * c] for c in range(C)]
    lay = W.planes_layout(ds, each)
    assert lay["keys"] == ["b", "m"]
    assert np.array_equal(lay["theta0"], [[1.0 + c, 2.0 * c] for c in range(C)])
    with pytest.raises(ValueError, match="one per walker"):
        W.planes_layout(ds, each[:-1])
    swapped = [list(p) for p in each]
    swapped[3] = [":m", 0.0, ":b", 1.0]
    with pytest.raises(ValueError, match="walker 3"):
        W.planes_layout(ds, swapped)


def test_the_x_mismatch_error_names_the_walker(W):
    ds = datasets()
    ds[2][0] = ds[2][0].copy()
    ds[2][0][4] = np.nextafter(ds[2][0][4], 10.0)     # one ulp: not "equal bit for bit"
    ds[4][0] = ds[4][0] + 1.0
    with pytest.raises(ValueError, match="walker 2"):
        W.planes_layout(ds, PARAMS)
    ds = [[np.zeros(N), np.ones(N)] for _ in range(C)]
    ds[1][0] = -ds[0][0]                               # -0.0 against +0.0: other bits
    with pytest.raises(ValueError, match="walker 1"):
        W.planes_layout(ds, PARAMS)
    ds = datasets()
    ds[3][0] = ds[3][0][:-1]
    with pytest.raises(ValueError, match="walker 3"):
        W.planes_layout(ds, PARAMS)
    ds = datasets()
    ds[3][1] = ds[3][1][:-1]
    with pytest.raises(ValueError, match="walker 3"):
        W.planes_layout(ds, PARAMS)


def test_data_separated_on_a_four_column_table(W):
    cols = [[1.0, 2.0, 3.0], [10.0, 20.0, 30.0], [11.0, 21.0, 31.0], [12.0, 22.0, 32.0]]
    sep = W.data_separated(cols)
    assert sep == [[cols[0], cols[1]], [cols[0], cols[2]], [cols[0], cols[3]]]
    assert all(s[0] is cols[0] for s in sep)
    lay = W.planes_layout(sep, PARAMS, [0.1, 0.2, 0.3])
    assert lay["y"].shape == (3, 3) and np.array_equal(lay["y"][2], cols[3])


def test_the_names_are_exported():
    import lisp_mcmc_amd as mhx
    for name in ("walker_set_create", "data_separated", "planes_layout"):
        assert name in mhx.__all__ and callable(getattr(mhx, name))
    assert (mhx.capi.SIGMA_NONE, mhx.capi.SIGMA_SHARED, mhx.capi.SIGMA_PER_CHAIN,
            mhx.capi.SIGMA_PER_POINT) == (0, 1, 2, 3)
    assert "mhx_set_dataset_planes" in mhx.capi.SIGNATURES
    assert "mhx_group_set_dataset_planes" in mhx.capi.SIGNATURES
