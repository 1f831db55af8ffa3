"""Column statistics and scale kernels (csrc/col_stats.h) on MI355X against
a reference on the exact (fp32- or bf16-rounded) data.

The reference sums are taken in numpy longdouble (64-bit significand), once
per case, so that the reference's own rounding (n * 2^-64) is invisible next
to the bounds, and every comparison is made in longdouble.

Bounds, with u = 2^-53: any-order fp64 summation of n exact terms is off by
at most (n - 1) u sum|term|, and the kernels' mean is (that sum) / n, one
more rounding; the test multiplies it by n exactly. So
|got - ref| <= n * 2^-52 * sum|term| for mean * n, norm_l1 and sumsq, with
nnz_j in place of n for CSR. The variance bound n * 2^-46 * (var + mean^2)
is the same bound with a 64x margin for the pivot and the merges; m2 of CSR
is held to n * 2^-46 * sumsq."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from asyncframework_amd import ops
from asyncframework_amd.ops import torch_ref

LD = np.longdouble
DTYPES = [torch.float32, torch.bfloat16]

# (rows, d): smallest; fewer rows than waves; flagship row on a ragged grid;
# ragged last block with several row slots per block; two column tiles and a
# 3-row last block; three column tiles; the generic form; more blocks (four
# column tiles) than rows
DENSE_SHAPES = [(1, 4), (3, 784), (1000, 784), (513, 260), (4099, 2048),
                (300, 2052), (500, 787), (2, 4096)]


def _core():
    assert ops.hip_available(), "HIP extension must be built on GPU boxes"
    import asyncframework_amd._hip_core as core
    return core


def _make_dense(n, d, dtype):
    """Columns offset + N(0,1) with offsets 0, 10, 1000 in turn; the last
    three columns are all zero, constant 0.1 and zero but for one entry."""
    g = torch.Generator().manual_seed(7 * d + n)
    X = torch.randn(n, d, generator=g)
    X += torch.tensor([0.0, 10.0, 1000.0])[torch.arange(d) % 3]
    X[:, d - 3] = 0.0
    X[:, d - 2] = 0.1
    X[:, d - 1] = 0.0
    X[n // 2, d - 1] = -2.5
    return X.to(dtype)


def _ref_stats(A):
    """longdouble two-pass statistics of the fp64 array A [n, d]."""
    n = A.shape[0]
    L = A.astype(LD)
    s = L.sum(0)
    mean = s / n
    m2 = ((L - mean) ** 2).sum(0)
    return dict(n=n, sum=s, mean=mean, m2=m2,
                var=m2 / (n - 1) if n > 1 else np.zeros_like(m2),
                l1=np.abs(L).sum(0), sumsq=(L * L).sum(0),
                nnz=(A != 0).sum(0), min=A.min(0), max=A.max(0))


_DENSE = {}


def _dense_case(n, d, dtype):
    key = (n, d, dtype)
    if key not in _DENSE:
        X = _make_dense(n, d, dtype)
        _DENSE[key] = dict(X=X, Xg=X.cuda(), ref=_ref_stats(
            X.double().numpy()))
    return _DENSE[key]


def _ld(t):
    return t.cpu().numpy().astype(LD)


def _ratio(err, bound):
    """max err / bound, 0 / 0 counting as 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))


def _check_stats(st, ref, count_for_sums, m2_bound, tag):
    n = ref["n"]
    assert st.count == n
    assert st.num_nonzeros.dtype == torch.int64
    assert st.num_nonzeros.cpu().tolist() == ref["nnz"].tolist()
    assert st.min.cpu().tolist() == ref["min"].tolist()
    assert st.max.cpu().tolist() == ref["max"].tolist()
    for t in (st.mean, st.m2, st.min, st.max, st.norm_l1, st.sumsq):
        assert t.dtype == torch.float64 and t.is_cuda
    k = count_for_sums.astype(LD) * LD(2.0) ** -52
    r_sum = _ratio(np.abs(_ld(st.mean) * n - ref["sum"]), k * ref["l1"])
    r_l1 = _ratio(np.abs(_ld(st.norm_l1) - ref["l1"]), k * ref["l1"])
    r_sq = _ratio(np.abs(_ld(st.sumsq) - ref["sumsq"]), k * ref["sumsq"])
    r_m2 = _ratio(*m2_bound(st))
    print(f"{tag}: err/bound sum {r_sum:.3e} l1 {r_l1:.3e} sumsq {r_sq:.3e} "
          f"var|m2 {r_m2:.3e}")
    assert r_sum <= 1.0 and r_l1 <= 1.0 and r_sq <= 1.0 and r_m2 <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", DENSE_SHAPES)
def test_dense_stats(shape, dtype):
    c = _dense_case(*shape, dtype)
    ref, (n, d) = c["ref"], shape
    st = ops.col_stats(c["Xg"])

    def var_bound(s):
        bound = n * LD(2.0) ** -46 * (ref["var"] + ref["mean"] ** 2)
        return np.abs(_ld(s.variance) - ref["var"]), bound

    _check_stats(st, ref, np.full(d, n), var_bound, f"{shape} {dtype}")
    # the all-zero and the constant column: exactly no spread
    assert float(st.m2[d - 3]) == 0.0 and float(st.m2[d - 2]) == 0.0
    again = ops.col_stats(c["Xg"])
    assert st.count == again.count
    for a, b in zip(st[1:], again[1:]):
        assert torch.equal(a, b)


def test_dense_grid_has_more_blocks_than_rows():
    g = _core().col_stats_geom(0, 2, 4096, 0)
    print(dict(g))
    assert g["vec"] == 4 and g["grid_x"] * g["grid_y"] > 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_unaligned_view_takes_the_generic_form(dtype):
    """d % 4 == 0 but the first element is one element past an aligned
    address: the 16-byte form must not be used."""
    c = _dense_case(513, 260, dtype)
    n, d = 513, 260
    buf = torch.zeros(n * d + 1, dtype=dtype, device="cuda")
    X = buf[1:].view(n, d)
    X.copy_(c["Xg"])
    assert _core().col_stats_geom(X.data_ptr(), n, d,
                                  int(dtype == torch.bfloat16))["vec"] == 1
    st, want = ops.col_stats(X), ops.col_stats(c["Xg"])
    for name in ("num_nonzeros", "min", "max"):
        assert torch.equal(getattr(st, name), getattr(want, name))
    assert torch.allclose(st.mean, want.mean, rtol=1e-12, atol=1e-15)
    assert torch.allclose(st.m2, want.m2, rtol=1e-9, atol=0.0)
    assert float(st.m2[d - 2]) == 0.0
    m = (torch.randn(d, generator=torch.Generator().manual_seed(1))).cuda()
    f = (torch.rand(d, generator=torch.Generator().manual_seed(2))).cuda()
    ops.scale_(X, m, f, with_mean=True)
    want = c["X"].clone()
    torch_ref.scale_(want, m.cpu(), f.cpu(), True)
    assert torch.equal(X.cpu(), want)
    assert float(buf[0]) == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 784), (513, 260), (500, 787)])
def test_dense_bounds(shape, dtype):
    """X is the head of a larger NaN buffer: the statistics read nothing
    past the last row, and the scale kernel writes nothing there."""
    c = _dense_case(*shape, dtype)
    n, d = shape
    big = torch.full((n + 5, d), float("nan"), dtype=dtype, device="cuda")
    big[:n] = c["Xg"]
    st, want = ops.col_stats(big[:n]), ops.col_stats(c["Xg"])
    for a, b in zip(st[1:], want[1:]):
        assert torch.equal(a, b)
    f = torch.full((d,), 0.5, device="cuda")
    ops.scale_(big[:n], torch.zeros(d, device="cuda"), f)
    assert bool(torch.isnan(big[n:]).all())
    assert bool(torch.isfinite(big[:n].float()).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_mean", [False, True])
@pytest.mark.parametrize("shape", [(1, 4), (3, 784), (513, 260),
                                   (300, 2052), (500, 787), (2, 4096)])
def test_scale_dense_is_bit_equal_to_the_reference(shape, with_mean, dtype):
    c = _dense_case(*shape, dtype)
    st = ops.col_stats(c["Xg"])
    from asyncframework_amd.data.scale import StandardScaler
    model = StandardScaler(with_mean=with_mean).fit(st)
    assert float(model.factor[shape[1] - 2]) == 0.0
    got = c["Xg"].clone()
    model.transform_(got)
    want = c["X"].clone()
    torch_ref.scale_(want, model.mean.cpu(), model.factor.cpu(), with_mean)
    assert torch.equal(got.cpu(), want)
    assert not torch.equal(got, c["Xg"])


# --------------------------------------------------------------------- CSR

def _csr_from_rows(cols, vals, dtype):
    indptr = np.zeros(len(cols) + 1, dtype=np.int32)
    indptr[1:] = np.cumsum([len(c) for c in cols])
    return (torch.from_numpy(indptr),
            torch.from_numpy(np.concatenate(cols).astype(np.int32)),
            torch.from_numpy(np.concatenate(vals)).float().to(dtype))


def _make_csr(n, d, per_row, dtype, special, empty_row):
    """About per_row entries a row with column-dependent offsets. With
    `special`: column 5 is empty, column 3 holds float32(0.1) and column 4
    holds 1 in every row; row 0 holds nothing else — and with `empty_row`
    nothing at all, so that the two columns then meet one implicit zero."""
    rng = np.random.default_rng(n + d)
    cols, vals = [], []
    for i in range(n):
        k = 0 if (special and i == 0) else max(1, rng.poisson(per_row))
        cc = np.sort(rng.choice(d, size=k, replace=False))
        vv = rng.standard_normal(k) + (cc % 3) * 10.0
        if special:
            keep = ~np.isin(cc, (3, 4, 5))
            cc, vv = cc[keep], vv[keep]
            if not (empty_row and i == 0):
                cc = np.concatenate([[3, 4], cc])
                vv = np.concatenate([[np.float32(0.1), 1.0], vv])
                o = np.argsort(cc)
                cc, vv = cc[o], vv[o]
        cols.append(cc)
        vals.append(vv)
    return _csr_from_rows(cols, vals, dtype)


_CSR = {}


def _csr_case(name, dtype):
    key = (name, dtype)
    if key not in _CSR:
        if name == "wide":
            n, d = 64, 47236
            indptr, indices, values = _make_csr(n, d, 75, dtype, False, False)
        else:
            n, d = 700, 300
            indptr, indices, values = _make_csr(n, d, 8, dtype, True,
                                                name == "empty_row")
        A = np.zeros((n, d))
        ip = indptr.numpy()
        for i in range(n):
            A[i, indices[ip[i]:ip[i + 1]].numpy()] = \
                values[ip[i]:ip[i + 1]].double().numpy()
        _CSR[key] = dict(n=n, d=d, cpu=(indptr, indices, values),
                         gpu=(indptr.cuda(), indices.cuda(), values.cuda()),
                         ref=_ref_stats(A))
    return _CSR[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["empty_row", "full", "wide"])
def test_csr_stats(name, dtype):
    """(700, 300) twice — a column can be full, or a row empty, not both:
    'empty_row' has row 0 empty, so columns 3 and 4 hold one implicit zero;
    in 'full' row 0 holds exactly those two entries and both columns are
    constant. 'wide' is (64, 47236)."""
    c = _csr_case(name, dtype)
    ref, n, d = c["ref"], c["n"], c["d"]
    st = ops.col_stats_csr(*c["gpu"], d)

    def m2_bound(s):
        return (np.abs(_ld(s.m2) - ref["m2"]),
                n * LD(2.0) ** -46 * ref["sumsq"])

    _check_stats(st, ref, ref["nnz"], m2_bound, f"{name} {dtype}")
    if name != "wide":
        assert int(st.num_nonzeros[5]) == 0 and float(st.m2[5]) == 0.0
        assert float(st.min[5]) == 0.0 and float(st.max[5]) == 0.0
    if name == "empty_row":
        assert c["cpu"][0][0] == c["cpu"][0][1]
        assert int(st.num_nonzeros[3]) == n - 1 and float(st.min[3]) == 0.0
        assert float(st.m2[4]) > 0.0
    if name == "full":
        assert int(st.num_nonzeros[3]) == n and int(st.num_nonzeros[4]) == n
        assert float(st.m2[3]) == 0.0 and float(st.m2[4]) == 0.0
    again = ops.col_stats_csr(*c["gpu"], d)
    for a, b in ((st.num_nonzeros, again.num_nonzeros), (st.min, again.min),
                 (st.max, again.max)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_csr_shard_and_out_of_range_columns(dtype):
    """A row shard (indptr not starting at 0, values a view into the whole)
    sees its own entries only; an entry whose column id is outside [0, d)
    is ignored by the statistics and left alone by the scale kernel."""
    c = _csr_case("full", dtype)
    indptr, indices, values = c["gpu"]
    d, cut = c["d"], 300
    st = ops.col_stats_csr(indptr[cut:].contiguous(), indices, values, d)
    base = int(indptr[cut])
    want = ops.col_stats_csr((indptr[cut:] - base).contiguous(),
                             indices[base:], values[base:], d)
    assert st.count == want.count == c["n"] - cut
    for name in ("num_nonzeros", "min", "max"):
        assert torch.equal(getattr(st, name), getattr(want, name))
    assert torch.allclose(st.sumsq, want.sumsq, rtol=1e-12)
    bad = indices.clone()
    bad[7], bad[11] = d, -1
    st = ops.col_stats_csr(indptr, bad, values, d)
    full = ops.col_stats_csr(indptr, indices, values, d)
    assert int(full.num_nonzeros.sum() - st.num_nonzeros.sum()) == 2
    v = values.clone()
    ops.scale_csr_(bad, v, torch.full((d,), 2.0, device="cuda"))
    assert v[7] == values[7] and v[11] == values[11]
    assert v[8] == (values[8].float() * 2.0).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["empty_row", "wide"])
def test_scale_csr_is_bit_equal_to_the_reference(name, dtype):
    c = _csr_case(name, dtype)
    from asyncframework_amd.data.scale import StandardScaler
    model = StandardScaler().fit(ops.col_stats_csr(*c["gpu"], c["d"]))
    _, indices, values = c["gpu"]
    got = values.clone()
    model.transform_csr_(indices, got)
    want = c["cpu"][2].clone()
    torch_ref.scale_csr_(c["cpu"][1], want, model.factor.cpu())
    assert torch.equal(got.cpu(), want)
    assert not torch.equal(got, values)


# --------------------------------------------------------------- the rest

def test_zero_rows_launch_nothing():
    st = ops.col_stats(torch.zeros(0, 8, device="cuda"))
    assert st.count == 0 and st.mean.is_cuda
    for t in st[1:]:
        assert t.tolist() == [0] * 8
    st = ops.col_stats_csr(torch.zeros(1, dtype=torch.int32, device="cuda"),
                           torch.zeros(0, dtype=torch.int32, device="cuda"),
                           torch.zeros(0, device="cuda"), 8)
    assert st.count == 0 and st.max.tolist() == [0.0] * 8


def test_col_stats_kernel_resources():
    """No kernel spills, and every one of them is reported."""
    info = _core().col_stats_kernel_info()
    names = list(info)
    assert sum(n.startswith("col_stats_dense_kernel<") for n in names) == 4
    assert sum(n.startswith("col_stats_csr_kernel<") for n in names) == 2
    assert sum(n.startswith("scale_dense_kernel<") for n in names) == 8
    assert sum(n.startswith("scale_csr_kernel<") for n in names) == 2
    assert "col_stats_finish_kernel" in names
    assert "col_stats_csr_finish_kernel" in names
    for name, e in info.items():
        print(name, dict(e))
        assert e["local_size_bytes"] == 0, (name, dict(e))
        assert e["max_active_blocks_per_cu"] >= 1, (name, dict(e))
        assert e["num_regs"] > 0
