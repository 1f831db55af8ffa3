"""Column statistics and the standard scaler on the CPU: the fp64 references
of ops/torch_ref.py against numpy two-pass, ColStats.merge, the scaler's
rules and the raw-space identity of unscale_weights."""

import numpy as np
import pytest
import torch

from asyncframework_amd import ops
from asyncframework_amd.data.scale import ScalerModel, StandardScaler

LOSS_RTOL, LOSS_ATOL = 1e-4, 1e-6  # the project's sweep bound


def _np_stats(A):
    """numpy fp64 two-pass statistics of the dense fp64 array A [n, d]."""
    n = A.shape[0]
    mean = A.sum(0) / n
    return dict(mean=mean, m2=((A - mean) ** 2).sum(0),
                nnz=(A != 0).sum(0), min=A.min(0), max=A.max(0),
                l1=np.abs(A).sum(0), sumsq=(A * A).sum(0))


def _check(st, ref, n, rtol=1e-12):
    assert st.count == n and isinstance(st.count, int)
    for name, got in (("mean", st.mean), ("m2", st.m2), ("l1", st.norm_l1),
                      ("sumsq", st.sumsq)):
        assert got.dtype == torch.float64, name
        scale = np.abs(ref[name]).max() + 1e-300
        np.testing.assert_allclose(got.numpy(), ref[name], rtol=rtol,
                                   atol=rtol * scale, err_msg=name)
    assert st.num_nonzeros.dtype == torch.int64
    assert st.num_nonzeros.tolist() == ref["nnz"].tolist()
    assert st.min.tolist() == ref["min"].tolist()
    assert st.max.tolist() == ref["max"].tolist()
    var = ref["m2"] / (n - 1) if n > 1 else np.zeros_like(ref["m2"])
    np.testing.assert_allclose(st.variance.numpy(), var, rtol=rtol,
                               atol=rtol * (np.abs(var).max() + 1e-300))
    np.testing.assert_allclose(st.std.numpy(), np.sqrt(var), rtol=rtol,
                               atol=1e-150)
    np.testing.assert_allclose(st.norm_l2.numpy(), np.sqrt(ref["sumsq"]),
                               rtol=rtol)


def _dense(n, d, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, generator=g)
    X[:, 1] += 10.0
    X[:, 2] += 1000.0
    if d > 5:
        X[:, 3] = 0.0
        X[:, 4] = 0.1
        X[:, 5] = 0.0
        X[n // 2, 5] = -3.0
    return X.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16,
                                   torch.float64])
@pytest.mark.parametrize("shape", [(1, 4), (2, 3), (257, 19)])
def test_dense_reference_matches_numpy(shape, dtype):
    X = _dense(*shape, dtype)
    st = ops.col_stats(X)
    _check(st, _np_stats(X.double().numpy()), shape[0])


def _csr_case(dtype=torch.float32):
    """(700, 30): ~8 non-zeros per row, row 0 empty, column 7 empty, column
    3 full of float32(0.1), column 4 full of ones except the empty row —
    so column 3 is not constant (row 0 holds an implicit zero) while a
    second matrix without the empty row makes both constant."""
    rng = np.random.default_rng(3)
    n, d = 700, 30
    A = np.zeros((n, d))
    for i in range(1, n):
        cols = rng.choice(d, size=8, replace=False)
        A[i, cols] = rng.standard_normal(8) + (cols % 3) * 5.0
        A[i, 3] = np.float32(0.1)
        A[i, 4] = 1.0
    A[:, 7] = 0.0
    A = torch.from_numpy(A).to(dtype).double().numpy()  # the rounded data
    return A


def _to_csr(A, dtype, drop_rows=()):
    rows = [i for i in range(A.shape[0]) if i not in drop_rows]
    indptr, idx, val = [0], [], []
    for i in rows:
        nz = np.nonzero(A[i])[0]
        idx.append(nz)
        val.append(A[i, nz])
        indptr.append(indptr[-1] + len(nz))
    return (torch.tensor(indptr, dtype=torch.int32),
            torch.from_numpy(np.concatenate(idx).astype(np.int32)),
            torch.from_numpy(np.concatenate(val)).to(dtype), A[rows])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_csr_reference_matches_numpy(dtype):
    A = _csr_case(dtype)
    indptr, indices, values, _ = _to_csr(A, dtype)
    st = ops.col_stats_csr(indptr, indices, values, A.shape[1])
    _check(st, _np_stats(A), A.shape[0])
    assert st.num_nonzeros[7] == 0 and st.m2[7] == 0.0
    assert st.min[7] == 0.0 and st.max[7] == 0.0
    assert st.min[3] == 0.0  # the empty row's implicit zero
    # without the empty row, columns 3 and 4 hold one value each
    indptr, indices, values, B = _to_csr(A, dtype, drop_rows=(0,))
    st = ops.col_stats_csr(indptr, indices, values, A.shape[1])
    _check(st, _np_stats(B), B.shape[0])
    assert st.m2[3] == 0.0 and st.m2[4] == 0.0
    assert st.variance[3] == 0.0 and st.variance[4] == 0.0


def test_csr_stored_zeros_are_skipped():
    """MultivariateOnlineSummarizer ignores a stored 0.0."""
    indptr = torch.tensor([0, 2, 3], dtype=torch.int32)
    indices = torch.tensor([0, 1, 1], dtype=torch.int32)
    values = torch.tensor([0.0, 2.0, 4.0])
    st = ops.col_stats_csr(indptr, indices, values, 3)
    assert st.num_nonzeros.tolist() == [0, 2, 0]
    assert st.mean.tolist() == [0.0, 3.0, 0.0]
    assert st.min.tolist() == [0.0, 2.0, 0.0]
    assert st.m2.tolist() == [0.0, 2.0, 0.0]


def test_csr_reference_agrees_with_dense_reference():
    A = _csr_case()
    indptr, indices, values, _ = _to_csr(A, torch.float32)
    sp = ops.col_stats_csr(indptr, indices, values, A.shape[1])
    de = ops.col_stats(torch.from_numpy(A).float())
    assert sp.count == de.count
    for a, b in zip(sp[1:], de[1:]):
        assert torch.allclose(a.double(), b.double(), rtol=1e-12, atol=1e-12)


def test_zero_rows():
    st = ops.col_stats(torch.zeros(0, 5))
    assert st.count == 0
    for t in st[1:]:
        assert t.tolist() == [0] * 5
    assert st.variance.tolist() == [0.0] * 5
    st = ops.col_stats_csr(torch.zeros(1, dtype=torch.int32),
                           torch.zeros(0, dtype=torch.int32),
                           torch.zeros(0), 5)
    assert st.count == 0 and st.min.tolist() == [0.0] * 5


def test_one_row_has_zero_variance():
    st = ops.col_stats(torch.tensor([[1.0, -2.0, 0.0]]))
    assert st.variance.tolist() == [0.0, 0.0, 0.0]
    assert st.mean.tolist() == [1.0, -2.0, 0.0]


@pytest.mark.parametrize("split", [0, 1, 2, 100, 256, 257])
def test_merge_of_two_halves_equals_the_whole(split):
    X = _dense(257, 19, torch.float32, seed=5)
    whole = ops.col_stats(X)
    got = ops.col_stats(X[:split]).merge(ops.col_stats(X[split:]))
    assert got.count == whole.count
    for name in ("mean", "m2"):
        a, b = getattr(got, name), getattr(whole, name)
        assert bool(((a - b).abs() <= 1e-12 * b.abs()).all()), name
    assert torch.equal(got.num_nonzeros, whole.num_nonzeros)
    assert torch.equal(got.min, whole.min)
    assert torch.equal(got.max, whole.max)
    assert torch.allclose(got.norm_l1, whole.norm_l1, rtol=1e-13)
    assert torch.allclose(got.sumsq, whole.sumsq, rtol=1e-13)
    # constant columns stay exactly constant through a merge
    assert got.m2[3] == 0.0 and got.m2[4] == 0.0


def test_merge_csr_chunks():
    A = _csr_case()
    indptr, indices, values, _ = _to_csr(A, torch.float32)
    d, cut = A.shape[1], 300
    base = int(indptr[cut])
    head = ops.col_stats_csr(indptr[:cut + 1], indices, values, d)
    tail = ops.col_stats_csr(indptr[cut:] - base, indices[base:],
                             values[base:], d)
    whole = ops.col_stats_csr(indptr, indices, values, d)
    got = head.merge(tail)
    assert got.count == whole.count
    assert torch.allclose(got.mean, whole.mean, rtol=1e-12, atol=1e-15)
    assert torch.allclose(got.m2, whole.m2, rtol=1e-12, atol=1e-15)
    assert torch.equal(got.min, whole.min)
    assert torch.equal(got.num_nonzeros, whole.num_nonzeros)


def test_constant_column_of_point_one():
    """n = 4099 copies of float32(0.1): raw moments in fp64 leave an M2 of
    1e-15..1e-9 here, i.e. a factor of 1e6 and more where MLlib gives 0."""
    X = torch.full((4099, 2), 0.1)
    X[:, 1] = torch.randn(4099, generator=torch.Generator().manual_seed(1))
    st = ops.col_stats(X)
    assert st.variance[0] == 0.0
    m = StandardScaler().fit(st)
    assert m.factor[0] == 0.0 and m.factor[1] > 0.0


def test_scaler_rules():
    X = _dense(257, 19, torch.float32, seed=2)
    st = ops.col_stats(X)
    m = StandardScaler().fit(st)
    assert m.factor.dtype == torch.float32 and m.mean.dtype == torch.float32
    assert m.mean.tolist() == [0.0] * 19 and not m.with_mean
    assert m.factor[3] == 0.0 and m.factor[4] == 0.0  # zero variance
    want = (1.0 / X.double().std(0, unbiased=True)).float()
    live = [j for j in range(19) if j not in (3, 4)]
    assert torch.allclose(m.factor[live], want[live], rtol=1e-6)
    ones = StandardScaler(with_std=False).fit(st)
    assert ones.factor.tolist() == [1.0] * 19
    both = StandardScaler(with_mean=True).fit(st)
    assert torch.equal(both.mean, st.mean.float())
    # min == max with a variance that rounding left non-zero is constant too
    bad = st._replace(m2=st.m2 + 1e-20)
    assert StandardScaler().fit(bad).factor[4] == 0.0


def test_with_mean_raises_where_it_cannot_work():
    st = ops.col_stats(_dense(50, 8, torch.float32))
    m = StandardScaler(with_mean=True).fit(st)
    with pytest.raises(ValueError):
        m.transform_csr_(torch.zeros(1, dtype=torch.int32), torch.ones(1))
    with pytest.raises(ValueError):
        m.unscale_weights(torch.ones(8))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_mean", [False, True])
def test_transform_is_the_fp32_arithmetic(dtype, with_mean):
    X = _dense(130, 19, dtype, seed=4)
    m = StandardScaler(with_mean=with_mean).fit(ops.col_stats(X))
    got = X.clone()
    assert m.transform_(got) is None
    x = X.float().numpy()
    want = ((x - m.mean.numpy()) * m.factor.numpy()).astype(np.float32)
    assert torch.equal(got, torch.from_numpy(want).to(dtype))
    if not with_mean and dtype == torch.float32:
        sd = got.double().std(0, unbiased=True)
        live = [j for j in range(19) if j not in (3, 4)]
        assert torch.allclose(sd[live], torch.ones(len(live),
                                                   dtype=torch.float64),
                              atol=1e-5)
        assert got[:, 4].abs().max() == 0.0


def test_transform_csr():
    A = _csr_case()
    indptr, indices, values, _ = _to_csr(A, torch.float32)
    m = StandardScaler().fit(ops.col_stats_csr(indptr, indices, values,
                                               A.shape[1]))
    got = values.clone()
    assert m.transform_csr_(indices, got) is None
    want = values.numpy() * m.factor.numpy()[indices.numpy()]
    assert torch.equal(got, torch.from_numpy(want.astype(np.float32)))


@pytest.mark.parametrize("objective", ["lsq", "logistic", "hinge"])
def test_unscaled_weights_score_the_raw_data(objective):
    """X_scaled @ w == X_raw @ unscale_weights(w), seen through the loss of
    ops.evaluate within the sweep bound."""
    g = torch.Generator().manual_seed(9)
    n, d = 400, 24
    X = torch.randn(n, d, generator=g) * (10.0 ** (torch.arange(d) % 4 - 1))
    X[:, 5] = 2.5  # a constant column: factor 0 on both sides
    y = (torch.rand(n, generator=g) > 0.5).float()
    W = torch.randn(3, d, generator=g) / d ** 0.5
    m = StandardScaler().fit(ops.col_stats(X))
    Xs = X.clone()
    m.transform_(Xs)
    a = ops.evaluate(Xs, y, W, objective).loss
    b = ops.evaluate(X, y, m.unscale_weights(W), objective).loss
    assert m.unscale_weights(W).dtype == torch.float32
    assert torch.allclose(a, b, rtol=LOSS_RTOL, atol=LOSS_ATOL), (a, b)


def test_standardize_uses_the_training_scaler_for_held_out_rows():
    from asyncframework_amd import run as runner
    g = torch.Generator().manual_seed(11)
    X = torch.randn(300, 6, generator=g) * torch.tensor(
        [1.0, 10.0, 0.1, 100.0, 1.0, 5.0])
    T = torch.randn(40, 6, generator=g) * 3.0
    y, yt = torch.zeros(300), torch.zeros(40)
    X0, T0 = X.clone(), T.clone()
    model = runner.standardize_((X, y), (T, yt), sparse=False)
    assert isinstance(model, ScalerModel)
    f = StandardScaler().fit(ops.col_stats(X0)).factor
    assert torch.equal(model.factor, f)
    assert torch.equal(X, X0 * f) and torch.equal(T, T0 * f)
