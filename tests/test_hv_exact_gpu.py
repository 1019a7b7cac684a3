"""``hv_exact.hip`` against the references of ``_hv_reference.py`` (MI355X, marked gpu): the numpy float64 form of the
contract's formulas, and exact rationals at n ≤ 64.

Bounds (``ops/hv.py``, u = 2⁻⁵³): a total is within (2n + 16)·u relative of the exact value at m ≤ 3, (3n + 16)·u at
m = 4; a contribution within (2n + 16)·u·vol(box i) absolute.  The numpy reference is within the same bounds, so against
it the tolerance is twice the bound; against the rationals it is the bound itself.

Shapes: n ∈ {1, 2, 63, 64, 65, 130, 257} crosses the chunk of 64 rows (the carry of the running maximum, a last partial
chunk); 4100 crosses the LDS tile of 2048 rows twice in the launches that tile (totals at m ≤ 3, contributions at
m = 2); the launches whose workgroup owns a slice set (total at m = 4, contributions at m = 3) hold all rows in one tile.
The fixtures hold an exact duplicate, rows tied in x, in z and in w, a dominated row, a zero and a negative coordinate.

Observed on an MI355X (gfx950), worst over the cases (the tests print every figure they assert):

==============================  ==============================================================
quantity                        worst observed
==============================  ==============================================================
total, from the exact value     0 at m = 2; 0.72·u at m = 3 (n = 63, bound 142·u); 0.69·u at
                                m = 4 (n = 2, bound 22·u)
total, from numpy float64       0 at m = 2; 1.98·u at (1500, 3) front (tolerance 6032·u);
                                7.15·u at (300, 4) uniform (tolerance 1832·u)
contributions, exact value      0 at m = 2; 0.37·u·vol(box i) at m = 3 (n = 2, bound 20)
contributions, numpy float64    0 at m = 2; 0.36·u·vol(box i) at (65, 3) (tolerance 292)
covered rows and empty boxes    exactly 0 in every case
reversed rows, CPU path         equal to the last bit on the 4-valued-x fixture at (257, m)
==============================  =============================================================="""
import numpy as np
import pytest
import torch

import _hv_reference as ref
from evoxmi.metrics import ExactHV
from evoxmi.ops import hv

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 130, 257]
CASES = [("fixture", n) for n in SIZES] + [("equal", 7), ("equal", 65)]
U = ref.U


def _dev(a):
    return torch.tensor(np.array(a)).cuda()


def _check_total(kind, n, m):
    p = ref.points(kind, n, m)
    got = hv.exact(_dev(p))
    assert got.shape == () and got.dtype == torch.float64 and got.is_cuda
    got, want, bound = float(got), ref.total_f64(kind, n, m), ref.total_bound(n, m)
    err = abs(got - want) / want if want else abs(got)
    print(f"[hv gpu] total {kind} ({n}, {m}): {err / U:.2f} u from float64 (tolerance {2 * bound / U:.0f} u)")
    assert err <= 2 * bound
    if n <= 64:
        e = ref.rel_err(got, ref.total_exact(kind, n, m))
        print(f"[hv gpu] total {kind} ({n}, {m}): {e / U:.2f} u from the exact value (bound {bound / U:.0f} u)")
        assert e <= bound


def _check_contributions(kind, n, m):
    p = ref.points(kind, n, m)
    got = hv.contributions(_dev(p))
    assert got.shape == (n,) and got.dtype == torch.float64 and got.is_cuda
    got, want, bound = got.cpu().numpy(), ref.contrib_f64(kind, n, m), ref.contrib_bound(p)
    vol = np.maximum(bound / ((2 * n + 16) * U), 1e-300)
    err = np.abs(got - want)
    print(f"[hv gpu] contributions {kind} ({n}, {m}): worst {np.max(err / vol) / U:.2f} u·vol from float64 (tolerance {2 * (2 * n + 16)})")
    assert np.all(err <= 2 * bound)
    if n <= 64:
        exact = ref.contrib_exact(kind, n, m)
        e = ref.abs_err(got, exact)
        print(f"[hv gpu] contributions {kind} ({n}, {m}): worst {np.max(e / vol) / U:.2f} u·vol from the exact value (bound {2 * n + 16})")
        assert np.all(e <= bound)
        zero = np.array([x == 0 for x in exact])
        assert np.all(got[zero] == 0.0) and np.all(got[~zero] > 0.0)
    if kind == "fixture" and n >= 7:
        assert got[1] == 0.0 and got[3] == 0.0 and got[4] == 0.0 and got[5] == 0.0  # duplicates, dominated, empty box
    if kind == "equal":
        assert np.all(got == 0.0)


@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("kind,n", CASES)
def test_total(kind, n, m):
    _check_total(kind, n, m)


@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("kind,n", CASES)
def test_contributions(kind, n, m):
    _check_contributions(kind, n, m)


@pytest.mark.parametrize("kind,n,m", [("front", 1500, 3), ("uniform", 1500, 3), ("front", 300, 4), ("uniform", 300, 4),
                                      ("uniform", 4100, 2), ("front", 4100, 3)])
def test_total_middle_sizes(kind, n, m):
    _check_total(kind, n, m)


@pytest.mark.parametrize("kind,n,m", [("front", 300, 3), ("uniform", 300, 3), ("front", 4100, 2), ("uniform", 4100, 2)])
def test_contributions_middle_sizes(kind, n, m):
    _check_contributions(kind, n, m)


@pytest.mark.parametrize("m", [2, 3, 4])
def test_ties_in_x_are_walked_as_on_the_cpu(m):
    n = 257
    p = ref.points("few_x", n, m)
    bound = ref.total_bound(n, m)
    a, b, c = float(hv.exact(_dev(p))), float(hv.exact(_dev(p[::-1].copy()))), float(hv.exact(torch.tensor(p)))
    print(f"[hv gpu] ties ({n}, {m}): reversed {abs(a - b) / a / U:.2f} u, cpu path {abs(a - c) / a / U:.2f} u (bound {bound / U:.0f} u)")
    assert abs(a - b) <= bound * a and abs(a - c) <= bound * a
    if m <= 3:
        ca, cb = hv.contributions(_dev(p)).cpu().numpy(), hv.contributions(_dev(p[::-1].copy())).cpu().numpy()[::-1]
        cc = hv.contributions(torch.tensor(p)).numpy()
        cbound = ref.contrib_bound(p)
        assert np.all(np.abs(ca - cb) <= cbound) and np.all(np.abs(ca - cc) <= cbound)


def test_two_calls_are_bitwise_equal():
    for m, n in ((2, 4100), (3, 1500), (4, 300)):
        x = _dev(ref.points("front" if m > 2 else "uniform", n, m))
        assert torch.equal(hv.exact(x), hv.exact(x))
    for m, n in ((2, 4100), (3, 300)):
        x = _dev(ref.points("front" if m == 2 else "uniform", n, m))
        assert torch.equal(hv.contributions(x), hv.contributions(x))


@pytest.mark.parametrize("m", [2, 3, 4])
def test_capture_and_replay(m):
    n = 257
    first, second = _dev(ref.points("fixture", n, m)), _dev(ref.points("few_x", n, m))
    with_c = m <= 3
    eager = [(hv.exact(x), hv.contributions(x) if with_c else None) for x in (first, second)]
    buf = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the capturing stream
        hv.exact(buf)
        if with_c:
            hv.contributions(buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tot = hv.exact(buf)
        con = hv.contributions(buf) if with_c else None
    for x, (et, ec) in ((second, eager[1]), (first, eager[0])):
        buf.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(tot, et)
        if with_c:
            assert torch.equal(con, ec)


def test_nothing_is_read_on_the_host(monkeypatch):
    xs = {m: _dev(ref.points("fixture", 130, m)) for m in (2, 3, 4)}
    for m, x in xs.items():  # warm-up: the extension is loaded
        hv.exact(x)
    torch.cuda.synchronize()

    def forbidden(*args, **kwargs):
        raise AssertionError("host read in the exact hypervolume")

    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "synchronize", forbidden)
        for name in ("item", "tolist", "cpu", "numpy", "__int__", "__bool__", "__float__", "__index__"):
            mp.setattr(torch.Tensor, name, forbidden)
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = [hv.exact(x) for x in xs.values()] + [hv.contributions(xs[2]), hv.contributions(xs[3])]
            out.append(ExactHV(torch.zeros(3, device="cuda"))(xs[3]))
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(o.is_cuda and o.dtype == torch.float64 for o in out)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_points_end_and_keep_the_shapes(bad):
    n = 130
    for m in (2, 3, 4):
        p = ref.points("fixture", n, m).copy()
        p[17, 1] = bad
        p[40, m - 1] = bad
        assert hv.exact(_dev(p)).shape == ()
        if m <= 3:
            assert hv.contributions(_dev(p)).shape == (n,)
    torch.cuda.synchronize()


def test_the_metric_stays_on_the_device():
    objs = torch.tensor([[1.0, 9], [2, 2], [3, 1]], device="cuda")
    m = ExactHV(torch.tensor([-1.0, -1], device="cuda"))
    got, c = m(objs), m.contributions(objs)
    assert got.is_cuda and c.is_cuda
    assert abs(float(got) - 25) <= 25e-12
    np.testing.assert_allclose(c.cpu().numpy(), [14.0, 1.0, 2.0], rtol=1e-12)
    assert hv.on_device(3, 2, objs.device) and not hv.on_device(2049, 4, objs.device)
    assert not hv.on_device(2049, 3, objs.device, contributions=True)
