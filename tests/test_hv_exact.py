"""``evoxmi.ops.hv`` on the CPU (its vectorised float64 torch path) and the metrics built on it, against the exact
rational reference of ``_hv_reference.py`` and against the host routine ``exact_hv``.

Bounds (the contract of ``ops/hv.py``, u = 2⁻⁵³): a total is within (2n + 16)·u relative of the exact value at m ≤ 3 and
(3n + 16)·u at m = 4; a contribution is within (2n + 16)·u·vol(box i) absolute; a row covered by another row gets 0.

Observed on the CPU path, worst over n ∈ {1, 2, 7, 33, 64} and the equal-rows fixture: totals 0, 1.48·u (n = 33) and
1.59·u (n = 64) relative at m = 2, 3, 4 (bounds 82·u and 208·u there); contributions 0 and 0.37 of u·vol(box i) at
m = 2, 3 (n = 2, bound 20).  At m = 2 every product and sum of these fixtures is exact.  Against ``exact_hv`` at
n = 40: 0, 1.8e-16 and 2.0e-16 relative (asked 1e-12); the leave-one-out differences at m = 3 use 0.35 of their
tolerance.  The duplicated, the dominated and the empty rows get exactly 0."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import _hv_reference as ref
from evoxmi import random as rnd
from evoxmi.metrics import HV, ExactHV, exact_hv, hv_contributions, hv_exact
from evoxmi.ops import hv

SIZES = [1, 2, 7, 33, 64]
CASES = [("fixture", n) for n in SIZES] + [("equal", 7)]


def _t(a):
    return torch.tensor(np.array(a))


@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("kind,n", CASES)
def test_total_against_the_exact_value(kind, n, m):
    p = ref.points(kind, n, m)
    got = hv.exact(_t(p))
    assert got.shape == () and got.dtype == torch.float64
    err, bound = ref.rel_err(float(got), ref.total_exact(kind, n, m)), ref.total_bound(n, m)
    print(f"[hv cpu] total {kind} ({n}, {m}): {err / ref.U:.2f} u relative (bound {bound / ref.U:.0f} u)")
    assert err <= bound


@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("kind,n", CASES)
def test_contributions_against_the_exact_value(kind, n, m):
    p = ref.points(kind, n, m)
    got = hv.contributions(_t(p))
    assert got.shape == (n,) and got.dtype == torch.float64
    exact = ref.contrib_exact(kind, n, m)
    err, bound = ref.abs_err(got.numpy(), exact), ref.contrib_bound(p)
    vol = np.maximum(bound / ((2 * n + 16) * ref.U), 1e-300)
    print(f"[hv cpu] contributions {kind} ({n}, {m}): worst {np.max(err / vol) / ref.U:.2f} u·vol (bound {2 * n + 16})")
    assert np.all(err <= bound)
    zero = np.array([e == 0 for e in exact])
    assert np.all(got.numpy()[zero] == 0.0)  # covered rows and empty boxes: exactly 0
    assert np.all(got.numpy()[~zero] > 0.0)


@pytest.mark.parametrize("m", [2, 3])
def test_duplicates_get_zero_and_exposed_rows_get_more(m):
    p = ref.points("fixture", 33, m)
    c = hv.contributions(_t(p)).numpy()
    assert c[1] == 0.0 and c[3] == 0.0  # rows 1 and 3 are equal
    assert c[4] == 0.0  # row 4 lies inside the box of row 2
    assert c[5] == 0.0  # a negative coordinate: an empty box
    q = np.maximum(p.astype(np.float64), 0.0)
    covered = np.array([any(j != i and np.all(q[j] >= q[i]) for j in range(len(q))) for i in range(len(q))])
    covered |= np.prod(q, axis=1) == 0.0  # an empty box has nothing to contribute
    assert covered[[1, 3, 4, 5]].all()
    assert np.all(c[~covered] > 0.0) and np.all(c[covered] == 0.0)
    e = hv.contributions(_t(ref.points("equal", 7, m))).numpy()
    assert np.all(e == 0.0)


@pytest.mark.parametrize("m", [2, 3, 4])
def test_total_agrees_with_the_host_routine(m):
    p = ref.uniform(40, m, seed=m)
    want = exact_hv(_t(p), torch.zeros(m))
    got = float(hv.exact(_t(p)))
    print(f"[hv cpu] against exact_hv at (40, {m}): {abs(got - want) / want:.2e} relative")
    assert abs(got - want) <= 1e-12 * want


@pytest.mark.parametrize("m", [2, 3])
def test_contributions_agree_with_leave_one_out_differences(m):
    n = 30
    p = ref.uniform(n, m, seed=10 + m)
    zero = torch.zeros(m)
    tot = exact_hv(_t(p), zero)
    loo = np.array([tot - exact_hv(_t(np.delete(p, i, 0)), zero) for i in range(n)])
    got = hv.contributions(_t(p)).numpy()
    tol = ref.contrib_bound(p) + 4 * ref.U * tot  # the bound, plus the rounding of a difference of two totals
    print(f"[hv cpu] against leave-one-out at ({n}, {m}): worst {np.max(np.abs(got - loo) / tol):.3f} of the tolerance")
    assert np.all(np.abs(got - loo) <= tol)


def test_float64_input_and_float32_input_give_the_same_value():
    p = ref.points("fixture", 33, 3)
    assert float(hv.exact(_t(p))) == float(hv.exact(_t(p).double()))


def test_outside_the_caps_is_an_error():
    with pytest.raises(ValueError, match="Monte-Carlo"):
        hv.exact(torch.zeros(4, 5))
    with pytest.raises(ValueError, match="exact_hv"):
        hv.exact(torch.zeros(4, 1))
    with pytest.raises(ValueError, match="2048"):
        hv.exact(torch.zeros(2049, 4))
    with pytest.raises(ValueError, match="2048"):
        hv.contributions(torch.zeros(2049, 3))
    with pytest.raises(ValueError, match="32768"):
        hv.exact(torch.zeros(32769, 3))
    with pytest.raises(ValueError):
        hv.contributions(torch.zeros(4, 4))
    with pytest.raises(ValueError):
        hv.exact(torch.zeros(5))
    assert hv.N_CAP == {2: 32768, 3: 32768, 4: 2048} and hv.N_CAP_CONTRIB == {2: 32768, 3: 2048}
    assert not hv.on_device(10, 3, "cpu")


def test_no_rows():
    for m in (2, 3, 4):
        z = hv.exact(torch.zeros(0, m))
        assert z.shape == () and z.dtype == torch.float64 and float(z) == 0.0
    for m in (2, 3):
        c = hv.contributions(torch.zeros(0, m))
        assert c.shape == (0,) and c.dtype == torch.float64
    assert float(ExactHV(torch.ones(3))(torch.zeros(0, 3))) == 0.0


def test_metric_on_the_fixtures_of_test_hv():
    ref2 = torch.tensor([-1.0, -1])
    objs = torch.tensor([[1.0, 9], [2, 2], [3, 1]])
    got = ExactHV(ref2)(objs)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64
    assert abs(float(got) - 25) <= 25e-12
    assert float(hv_exact(objs, ref2)) == float(got)
    c = ExactHV(ref2).contributions(objs)
    assert torch.equal(c, hv_contributions(objs, ref2))
    np.testing.assert_allclose(c.numpy(), [14.0, 1.0, 2.0], rtol=1e-12)  # by hand: boxes (2, 10), (3, 3), (4, 2)
    ref3 = torch.tensor([10, 9, 8.0])
    objs = torch.tensor([[0.1, 7, 0.3], [5.5, 0, 2.3], [-0.1, 1, -1], [3, 2, 5.5]])
    assert abs(float(ExactHV(ref3)(objs)) - 753) < 2
    # exact_hv subtracts in float64, the metric in the dtype of objs: compare on the same float32 points
    assert abs(float(ExactHV(ref3)(objs)) - exact_hv(torch.abs(objs - ref3), torch.zeros(3))) <= 1e-12 * 753


def test_metric_agrees_with_the_estimator_in_4d():
    g = torch.Generator().manual_seed(0)
    objs = torch.rand(12, 4, generator=g)
    ref4 = torch.ones(4) * 1.1
    ex = float(ExactHV(ref4)(objs))
    mc = float(HV(ref4, 400_000, "bounding_cube")(rnd.PRNGKey(1), objs))
    assert abs(mc - ex) / ex < 0.02
    assert abs(ex - exact_hv(torch.abs(objs - ref4), torch.zeros(4))) <= 1e-12 * ex


def test_the_references_agree_with_each_other():
    for m in (2, 3, 4):
        p = ref.points("fixture", 33, m)
        assert ref.rel_err(ref.hv_numpy(p), ref.total_exact("fixture", 33, m)) <= ref.total_bound(33, m)
    for m in (2, 3):
        p = ref.points("fixture", 33, m)
        err = ref.abs_err(ref.contributions_numpy(p), ref.contrib_exact("fixture", 33, m))
        assert np.all(err <= ref.contrib_bound(p))
    assert ref.hv_fraction(np.array([[1.0, 2.0, 3.0], [2.0, 1.0, 1.0]], np.float32)) == Fraction(7)
