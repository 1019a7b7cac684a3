"""``moead_small_ask`` / ``moead_small_tell`` (``moead_small.hip``) and ``BatchedRuns(MOEAD)`` on an MI355X: ask and tell bit for bit
against the solo ops with every run's operands, tell also against ``_moead_reference.replace_ref`` (float64; each case first asserts
the reference's 64-ulp margin on the CPU, no case skipped; ``z_max`` is no output and is pinned through ``tchebycheff_norm``)."""
import functools

import pytest
import torch

import _moead_reference as ref
from evoxmi.algorithms.containers.batched import BatchedRuns
from evoxmi.algorithms.mo.moead import reverse_neighbors
from evoxmi.ops import mo as mo_ops
from evoxmi.ops import random as rnd
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

from test_batched_ibea_spea2 import same_bits
from test_batched_ibea_spea2_gpu import ext  # noqa: F401
from test_batched_moead import D, FUNCS, M, POP, check_moead_runs_equal_solo, make

pytestmark = pytest.mark.gpu
RATES = (0.6, 20.0, 2.0, 20.0)  # pro_c < 1: rows without crossover occur


def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(v) * 10007**k for k, v in enumerate(seed)) + 1)


def _neighbors(R, N, T, g):
    row = lambda: torch.randperm(N, generator=g)[:T] if T <= N else torch.randint(0, N, (T,), generator=g)  # noqa: E731
    return torch.stack([torch.stack([row() for _ in range(N)]) for _ in range(R)])


# ---------------------------------------------------------------- ask
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("d", [1, 4, 37, 64, 260])  # 260: a second pass of the lanes over the row, float4
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 129])
@pytest.mark.parametrize("N", [1, 5, 91])
def test_ask_equals_solo_ops(ext, N, T, d, R):
    g = _gen(1, N, T, d, R)
    shared = d in (4, 37)
    nb = _neighbors(1 if shared else R, N, T, g)
    lb = torch.rand(d, generator=g) - 2
    ub = lb + torch.tensor([1e-3, 1.0, 4.0, 1e3])[torch.randint(0, 4, (d,), generator=g)]
    pop = (lb + torch.rand(R, N, d, generator=g) * (ub - lb)).cuda()
    keys = torch.stack([rnd.split(rnd.PRNGKey(N + 7 * T + 31 * d + r), 3) for r in range(R)]).cuda()  # (R, 3, 2): parent, SBX, PM
    off, par = mo_ops.moead_small_ask(pop, nb.cuda(), keys[:, 0].contiguous(), keys[:, 1], keys[:, 2], lb.cuda(), ub.cuda(), *RATES)
    assert off.shape == (R, N, d) and par.shape == (R, 2, N) and par.dtype == torch.int32
    for r in range(R):
        nbr = nb[0 if shared else r]
        p0, p1 = mo_ops.moead_parents(nbr.cuda(), keys[r, 0])
        assert torch.equal(par[r], torch.stack([p0, p1])) and torch.equal(par[r].cpu().long(), torch.stack(ref.parents_ref(nbr, keys[r, 0].cpu())))
        assert same_bits(off[r], mo_ops.moead_variation(pop[r], p0, p1, keys[r, 1], keys[r, 2], lb.cuda(), ub.cuda(), *RATES)), f"run {r}"
    if R == 1:  # operands without a run axis are one run
        o2, p2 = mo_ops.moead_small_ask(pop[0], nb[0].cuda(), keys[0, 0], keys[0, 1], keys[0, 2], lb.cuda(), ub.cuda(), *RATES)
        assert same_bits(o2, off[0]) and torch.equal(p2, par[0])


# ---------------------------------------------------------------- tell
@functools.lru_cache(maxsize=None)
def _tell_case(N, m, d, func, R=3, shared=False):
    """z[0] lies above the offspring (z' takes their minimum there); occupants: the slot's best offspring × 1.05 or 0.95."""
    g = _gen(2, N, m, d)
    T = max(1, min(N, (N + 9) // 10 + 2))
    nb = _neighbors(1 if shared else R, N, T, g).expand(R, N, T)
    W = (torch.rand(1 if shared else R, N, m, generator=g) + 0.05).expand(R, N, m)
    off_obj, off, pop = torch.rand(R, N, m, generator=g), torch.rand(R, N, d, generator=g) + 2, torch.rand(R, N, d, generator=g)
    z = torch.full((R, m), -0.01) - 0.01 * torch.rand(R, m, generator=g)
    z[:, 0] = 10.0
    z2 = torch.minimum(z, off_obj.min(1).values)
    csr = [reverse_neighbors(nb[r]) for r in range(R)]
    far = torch.full((N, m), 1e6)
    best = torch.stack([ref.replace_ref(far, off_obj[r], W[r], z2[r], far.max(0).values, csr[r][0], csr[r][2], func)[0] for r in range(R)])
    scale = torch.where(torch.rand(R, N, 1, generator=g) < 0.5, 1.05, 0.95)
    pop_obj = torch.where((best >= 0)[..., None], torch.stack([off_obj[r][best[r].clamp_min(0)] for r in range(R)]) * scale,
                          torch.rand(R, N, m, generator=g))
    return dict(pop=pop, off=off, pop_obj=pop_obj, off_obj=off_obj, W=W, nb=nb, z=z, z2=z2, csr=csr, shared=shared)


def _small_tell(c, func):
    lead = lambda t: t[:1] if c["shared"] else t  # noqa: E731
    out = mo_ops.moead_small_tell(c["pop"].cuda(), c["off"].cuda(), c["pop_obj"].cuda(), c["off_obj"].cuda(), lead(c["W"]).cuda(),
                                  lead(c["nb"]).cuda(), c["z"].cuda(), func)
    assert out[3].dtype == torch.int32 and out[3].shape == c["pop"].shape[:2]
    return out


def _same_as_solo_ops(c, func):
    """Every run against torch's reference points, the CSR, ``moead_replace`` and ``moead_select_rows`` on the device."""
    got = _small_tell(c, func)
    for r in range(c["pop"].shape[0]):
        dev = lambda k: c[k][r].cuda().contiguous()  # noqa: E731
        z2 = torch.minimum(dev("z"), dev("off_obj").min(0).values)
        rowptr, _, owner = reverse_neighbors(dev("nb"))
        win, new_obj = mo_ops.moead_replace(dev("pop_obj"), dev("off_obj"), dev("W"), z2, dev("pop_obj").max(0).values, rowptr.int(), owner.int(), func)
        for g, w in zip(got, (mo_ops.moead_select_rows(dev("pop"), dev("off"), win), new_obj, z2, win)):
            assert same_bits(g[r], w), f"run {r}"
    return got


@pytest.mark.parametrize("N", [1, 5, 91, 300])
@pytest.mark.parametrize("func", FUNCS)
@pytest.mark.parametrize("m", [1, 2, 3, 5, 16])
def test_tell_against_float64_reference(ext, m, func, N):
    c = _tell_case(N, m, 5, func, shared=(m == 5))
    want = []
    for r in range(3):
        win, new_obj, info = ref.replace_ref(c["pop_obj"][r], c["off_obj"][r], c["W"][r], c["z2"][r], c["pop_obj"][r].max(0).values,
                                             c["csr"][r][0], c["csr"][r][2], func)
        assert info["margin"] >= 64 and info["ties_occupant"] == 0, info
        want.append((torch.where((win >= 0)[:, None], c["off"][r][win.clamp_min(0)], c["pop"][r]), new_obj, c["z2"][r], win.int()))
    assert N < 91 or all(0.2 <= float((w[3] >= 0).float().mean()) <= 0.8 for w in want)  # slots replace and slots keep
    got = _small_tell(c, func)
    for k, name in enumerate(("new_pop", "new_obj", "z'", "win")):
        assert same_bits(got[k].cpu(), torch.stack([w[k] for w in want])), name


@pytest.mark.parametrize("func", FUNCS)
@pytest.mark.parametrize("N,m,d", [(91, 3, 12), (300, 3, 30), (300, 16, 7), (2048, 16, 4)])  # staged and unstaged objectives; the cap
def test_tell_equals_solo_ops(ext, N, m, d, func):
    c = _tell_case(N, m, d, "weighted_sum", R=2)  # occupants near the weighted-sum optimum: every func replaces some slots
    got = _same_as_solo_ops(c, func)
    assert bool((got[3] >= 0).any()) and bool((got[3] < 0).any())


EDGES = [("tie", "pbi"), ("tie", "tchebycheff"), ("equal_occupant", "tchebycheff"), ("equal_occupant", "tchebycheff_norm"),
         ("signed_zero", "weighted_sum"), ("nan_offspring", "weighted_sum"), ("nan_offspring", "tchebycheff"), ("nan_occupant", "pbi"),
         ("inf_offspring", "modified_tchebycheff"), ("inf_offspring", "weighted_sum")]


@pytest.mark.parametrize("case,func", EDGES)
def test_tell_edges_follow_the_solo_ops(ext, case, func):
    """The expected values are the solo ops'.  ``signed_zero``: rows of −0.0 and of +0.0 objectives bid for the same slots; both
    weighted sums are +0 (``agg`` adds onto +0), and no aggregation gives one slot candidates of both signs of zero: the kernel's
    fold of −0 keeps the packed order equal to the float order, and nothing observable depends on it."""
    c = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in _tell_case(16, 3, 5, "weighted_sum", R=2).items()}
    c["z"][:, 0] = -0.02
    star = c["z"] + 1e-4  # beats every row drawn from [0, 1)
    c["nb"][:, 7] = c["nb"][:, 3]  # offspring 3 and 7 bid for the same slots
    slot = c["nb"][0, 3, 0]
    c["off_obj"][:, 3] = {"signed_zero": torch.zeros_like(star), "inf_offspring": star + float("inf")}.get(case, star)
    if case == "tie":
        c["off_obj"][:, 7] = star
    elif case == "signed_zero":
        c["off_obj"][:, 7] = -0.0
    elif case == "nan_offspring":
        c["off_obj"][:, 3, 1] = float("nan")  # with tchebycheff the NaN column of z' stops every replacement
    elif case == "equal_occupant":
        c["pop_obj"][0, slot] = star[0]
    elif case == "nan_occupant":
        c["pop_obj"][0, slot, 0] = float("nan")
    assert bool((_same_as_solo_ops(c, func)[3] == 3).any()) == (case not in ("nan_offspring", "inf_offspring"))


# ---------------------------------------------------------------- BatchedRuns, dispatch, caps
@pytest.mark.parametrize("func", ["pbi", "tchebycheff_norm"])
def test_batched_moead_runs_equal_solo_gpu(ext, func):
    check_moead_runs_equal_solo(func, "cuda", runs=4)


def test_batched_moead_captured_equals_eager(ext):
    def final(graph):
        wf = StdWorkflow(BatchedRuns(make("pbi", "cuda"), 4), DTLZ2(d=D, m=M), graph=graph)
        st = wf.init(rnd.PRNGKey(9, device="cuda"))
        for _ in range(6):  # the initial evaluation, then five generations: several replays
            st = wf.step(st)
        runs = st.get_child_state("algorithm").runs
        return [runs[k].clone() for k in ("population", "fitness", "z", "win", "parents", "key")]

    assert all(same_bits(a, b) for a, b in zip(final(False), final(True)))


def test_vmapped_calls_are_the_batched_launches_and_caps_raise(ext):
    from torch.func import vmap
    from torch.utils._python_dispatch import TorchDispatchMode

    from evoxmi.ops import batching

    class Calls(TorchDispatchMode):
        names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(func.name())
            return func(*args, **(kwargs or {}))

    batching.register()
    c = _tell_case(POP, 3, 12, "pbi")
    args = [c[k].cuda() for k in ("pop", "off", "pop_obj", "off_obj", "W", "nb", "z")]
    keys = torch.stack([rnd.split(rnd.PRNGKey(r), 3) for r in range(3)]).cuda()
    lb, ub = torch.zeros(12).cuda(), torch.ones(12).cuda()
    ask = lambda p, nb, k, lo: mo_ops.moead_small_ask(p, nb, k[0], k[1], k[2], lo, ub, *RATES)  # noqa: E731
    with Calls() as calls:
        got = vmap(lambda *a: mo_ops.moead_small_tell(*a, "pbi"))(*args)
        per_run = vmap(ask, in_dims=(0, 0, 0, None))(args[0], args[5], keys, lb)
        shared = vmap(ask, in_dims=(0, 0, 0, None))(args[0], args[5][:1].expand(3, -1, -1), keys, lb)  # stride 0: what vmap(init) leaves
        const = vmap(ask, in_dims=(0, None, 0, None))(args[0], args[5][0], keys, lb)
    assert calls.names.count("evoxmi::moead_small_tell") == 1 and calls.names.count("evoxmi::moead_small_ask") == 3, calls.names
    assert all(same_bits(g, w) for g, w in zip(got, mo_ops.moead_small_tell(*args, "pbi")))
    assert all(same_bits(a, b) and same_bits(a, w) for a, b, w in zip(shared, const, ask(args[0], args[5][:1], keys.transpose(0, 1), lb)))
    assert same_bits(per_run[0][0], shared[0][0]) and not same_bits(per_run[0][1], shared[0][1])
    with pytest.raises(NotImplementedError, match="bounds"):
        vmap(ask, in_dims=(0, 0, 0, 0))(args[0], args[5], keys, lb.expand(3, 12))
    for n, m in ((2049, 3), (4, 17)):
        big = [torch.zeros(2, n, 4), torch.zeros(2, n, 4), torch.zeros(2, n, m), torch.zeros(2, n, m), torch.ones(2, n, m),
               torch.zeros(2, n, 1, dtype=torch.int64), torch.zeros(2, m)]
        with pytest.raises(NotImplementedError, match="2048"):
            vmap(lambda *a: mo_ops.moead_small_tell(*a, "pbi"))(*(t.cuda() for t in big))
