"""BCE-IBEA's PC selection and exploration on the CPU: the numpy float64 references of ``_bce_reference.py``
against the torch expressions, ``ops/bce.py``'s CPU entries against ``bce_ibea.py``'s functions bit for bit, the
fixed-shape odd branch against the ``nonzero`` one, and the generation parity the workflow hands to ``ask``.

The torch expressions evaluate in float32 and normalise before they subtract, so they are pinned to the float64
reference only where the reference's own margins are wide: the removal order where its smallest relative gap
between the two least products is at least 1e-3 (asserted), the exploration mask outside the rows that have an NPC
distance within 1e-4 relative of the radius."""
import numpy as np
import pytest
import torch

import _bce_reference as ref
import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.algorithms.mo import bce_ibea as bce_mod
from evoxmi.ops import bce as bce_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow


# ---------------------------------------------------------------- the references
@pytest.mark.parametrize("n,m,seed", [(24, 2, 0), (40, 3, 1), (40, 3, 2), (33, 5, 4)])
def test_reference_removal_is_the_torch_pc_selection(n, m, seed):
    obj = ref.objectives(n, m, "front", seed)
    mask = ref.nd_mask(obj)
    assert mask.all()
    n_keep = n // 2
    order, gap, ties_ok, ties, factors, _ = ref.removal(obj, mask, n - n_keep)
    print(f"[pin] ({n}, {m}) seed {seed}: gap {gap:.3e}, ties {ties}, factors {factors}")
    assert gap >= 1e-3 and ties_ok
    xs = []
    idx, n_nd = bce_ops.pc_selection_indices(torch.tensor(obj), n_keep, xs)
    assert n_nd == n and xs == order.tolist()
    assert np.array_equal(idx.numpy(), ref.select_indices(n, mask, order, n_keep))


def test_reference_mask_and_radius_are_the_torch_ones():
    obj = ref.objectives(60, 3, "uniform", 5)
    mask = ref.nd_mask(obj)
    assert 3 < mask.sum() < 60
    idx, n_nd = bce_ops.pc_selection_indices(torch.tensor(obj), 60)
    assert n_nd == int(mask.sum()) and np.array_equal(idx.numpy()[:n_nd], np.flatnonzero(mask))
    t, r, _ = ref.niche(obj, mask)
    r32, t32 = bce_ops.niche_radius(torch.tensor(obj), torch.tensor(mask))
    assert np.allclose(t32.numpy(), t, rtol=1e-4, atol=1e-6) and abs(float(r32) - r) <= 1e-4 * r


@pytest.mark.parametrize("n,m,seed", [(30, 2, 0), (50, 3, 1), (64, 5, 2)])
def test_reference_exploration_is_the_torch_exploration(n, m, seed):
    pc = ref.objectives(n, m, "front", seed)
    rng = np.random.default_rng(100 + seed)
    npc = (ref.objectives(n, m, "front", 50 + seed) * (1 + 0.05 * rng.random((n, 1)))).astype(np.float32)
    for n_nd in (n, n // 2):
        want, near = ref.exploration(pc, npc, n_nd)
        got = bce_mod.exploration(torch.tensor(pc), torch.tensor(npc), n_nd, n).numpy()
        assert near.sum() <= 1 and np.array_equal(got[~near], want[~near])
        assert 0 < want.sum() < n or n_nd != n


# ---------------------------------------------------------------- ops/bce.py on the CPU
@pytest.mark.parametrize("kind,n,n_keep", [("front", 40, 20), ("front", 41, 40), ("uniform", 60, 30), ("uniform", 60, 5)])
def test_pc_select_on_the_cpu_is_pc_selection_bit_for_bit(kind, n, n_keep):
    obj = torch.tensor(ref.objectives(n, 3, kind, 7))
    pop = torch.arange(n, dtype=torch.float32)[:, None].repeat(1, 4)
    pc, pc_obj, n_nd = bce_mod.pc_selection(pop, obj, n_keep)
    idx, n_nd2 = bce_ops.pc_select(obj, n_keep)
    assert idx.dtype == torch.int64 and idx.shape == (n_keep,) and n_nd2.dtype == torch.int64 and n_nd2.dim() == 0
    assert int(n_nd2) == n_nd and torch.equal(pop[idx], pc) and torch.equal(obj[idx].view(torch.int32), pc_obj.view(torch.int32))
    if kind == "uniform" and n_keep == 30:  # the padding case: fewer non-dominated rows than places
        assert n_nd < n_keep and torch.equal(idx[n_nd:], idx[:1].expand(n_keep - n_nd))
    idx3, _, order, rescans = bce_ops.pc_select(obj, n_keep, return_order=True)
    k = max(0, n_nd - n_keep)
    assert torch.equal(idx3, idx) and order.shape == (n - n_keep,) and int(rescans) == 0
    assert (order[k:] == -1).all() and len(set(order[:k].tolist())) == k and not set(order[:k].tolist()) & set(idx.tolist())


def test_explore_on_the_cpu_is_exploration():
    pc, npc = torch.tensor(ref.objectives(30, 3, "front", 1)), torch.tensor(ref.objectives(30, 3, "front", 2))
    assert torch.equal(bce_ops.explore(pc, npc, 17, 30), bce_mod.exploration(pc, npc, 17, 30))
    assert bce_mod.exploration is bce_ops.exploration


# ---------------------------------------------------------------- the algorithm
def _nonzero_ask(algo, state):
    """The odd branch as it was: candidates by ``nonzero``, the population kept where there is none."""
    key, k1, x_key, mut_key = rnd.split(state.key, 4)
    N = algo.pop_size
    s = bce_mod.exploration(state.fitness, state.npc_obj, state.n_nd, N)
    if bool(s.any()):
        cand = torch.nonzero(s).flatten()
        mate = rnd.randint(k1, (N,), 0, N).to(cand.device)
        first = cand[torch.arange(N, device=cand.device) % cand.shape[0]]
        parents = torch.cat([state.population[first], state.population[mate]])
        off = algo.mutation(mut_key, algo.crossover_odd(x_key, parents))
    else:
        off = state.population.clone()
    return torch.clamp(off, algo.lb, algo.ub), key, bool(s.any())


def _workflow(d=6, m=3, pop=20):
    algo = A.BCEIBEA(torch.zeros(d), torch.ones(d), m, pop)
    wf = StdWorkflow(algo, DTLZ2(d=d, m=m))
    return algo, wf, wf.init(rnd.PRNGKey(3))


def test_fixed_shape_odd_branch_is_the_nonzero_branch():
    algo, wf, st = _workflow()
    seen = 0
    for _ in range(5):
        st = wf.step(st)
        a = st.get_child_state("algorithm")
        if a.counter % 2 == 1:
            want, key, any_s = _nonzero_ask(algo, a)
            off, b = algo.ask(a)
            assert torch.equal(off, want) and torch.equal(b.key, key)
            seen += any_s
    assert seen >= 1  # a step with candidates
    # no candidate: every PC row has the whole of NPC inside its (zero) radius
    same = torch.full_like(a.fitness, 0.5)
    c = a.update(fitness=same, npc_obj=same.clone(), counter=1)
    assert not bool(bce_mod.exploration(c.fitness, c.npc_obj, c.n_nd, algo.pop_size).any())
    want, key, any_s = _nonzero_ask(algo, c)
    off, b = algo.ask(c)
    assert not any_s and torch.equal(off, want) and torch.equal(off, torch.clamp(c.population, algo.lb, algo.ub))
    assert torch.equal(b.key, key)


def test_variant_parity_is_the_counter_parity():
    algo, wf, st = _workflow()
    assert set(algo.graph_variant_set()) == {"explore", "ibea"}
    for step in range(7):
        gen = int(st.generation)
        if gen >= 1:
            counter = int(st.get_child_state("algorithm").counter)
            assert counter == gen
            variant = algo.graph_variant(gen)
            assert variant == ("explore" if counter % 2 else "ibea")
            with algo.graph_variant_context(variant):
                assert algo._parity == counter % 2
            assert algo._parity is None
        st = wf.step(st)
    assert int(st.generation) == 7
