"""vmap rules that fold a batch of independent runs into ONE launch of each HIP op.

``BatchedRuns`` (``evoxmi/algorithms/containers/batched.py``) executes n independent
runs of an algorithm under ``torch.func.vmap``.  PyTorch's own ops batch natively; the
evoxmi HIP ops below would otherwise hit functorch's per-sample fallback (one launch
per run).  Each rule moves the run axis to the front and calls the op's batched form:

* ``philox_words`` / ``philox_fill``: keys (B, 2) → grid.y = run (``rng.hip``);
* ``rank_argsort_f32``: keys (B, n) → grid.y = run, a row of workgroups per run (``sort.hip``).
  The rule is the public op's batched form; ``evoxmi.ops.sort`` itself sends batched keys to
  ``torch.sort``;
* ``de_trial``: P (B, rows, d), idx (B, R, K), per-row vectors (B, R), keys (B, 2) →
  grid.y = run, all indices run-local (``evo_ops.hip``);
* ``sbx`` / ``pm``: x (B, n, d), keys (B, 2, 2) → grid.y = run, run-local row counters, bounds shared
  (``evo_ops.hip``);
* ``nds``: f (B, n, m) → one workgroup per run (``nds_batched.hip``; n ≤ 8192, m ≤ 8 per run);
* ``nsga_select``: rank (B, n), f (B, n, m) → one workgroup per run (``nsga_select.hip``);
* ``ibea_fitness`` / ``spea2_fitness``: obj (B, n, m) → grid.y = run (``ibea_select.hip``, ``spea2_select.hip``; m ≤ 16, for
  SPEA2 n ≤ 32768 per run);
* ``ibea_truncate`` / ``spea2_truncate``: obj (B, n, m), per-row operands (B, n) → one workgroup per run, whose removal loop
  is the single-run one (n ≤ 8192, m ≤ 16 per run); SPEA2's runs each count their own removals;
* ``cma_small_ask`` / ``cma_small_tell``: every state field (B, …) → one workgroup per run (``cma_small.hip``; d ≤ 64, λ ≤ 1024
  per run), the recombination weights and the constants shared by the runs;
* ``moead_small_ask``: pop (B, N, d), keys (B, 2) and (B, 2, 2) → a wave per offspring, grid.y = run; ``moead_small_tell``: pop, off
  (B, N, d), objectives (B, N, m), z (B, m) → one workgroup per run (``moead_small.hip``; N ≤ 2048, m ≤ 16 per run).  The neighbour
  table and the weights may be shared by the runs or per run; the bounds and the rates are shared;
* ``nsga3_associate``: f (B, n, m), rank (B, n) → one workgroup per run normalises, grid.y = run associates
  (``nsga3_assoc.hip``; n ≤ 8192, m ≤ 16, K ≤ 8192 per run), the reference points shared by the runs; ``nsga3_niche_select``:
  rank, group, group_dist (B, n), last_rank (B,), keys (B, 2) → one workgroup per run (``nsga3_select.hip``);
* ``hype_fitness``: points (B, n, m), ref (B, m), keys (B, 2) → grid.y = run in both kernels (``hype_fitness.hip``; n ≤ 2048, m ≤ 16,
  n_sample ≤ 2^20 per run), α shared by the runs.  ``hv_count`` and ``hv_contrib`` have no batched form: their rules pass unbatched
  calls through and raise on batched operands (``tests/test_hype_fitness_gpu.py``);
* ``rvea_select``: f (B, n, m), shift (B, m), v (B, nv, m), θ (B,) → ``rvea_small_select``, one workgroup per run that keeps the run's
  normalised vectors in LDS (``rvea_small.hip``; n ≤ 4096 and nv ≤ 2048, 1024 or 512 for m ≤ 4, 8 or 16 per run); an unbatched
  operand is broadcast.  Every output of run r is the 2-D op's on that run, bit for bit (``tests/test_batched_rvea_gpu.py``).
  ``rvea_cos_best`` has no batched form: its rule passes unbatched calls through and raises on batched operands.;
* ``tdea_theta_rank``: obj (B, n, m), mask (B, n), w (nw, m) or (B, nw, m), θ (nw,) or (B, nw) → ``tdea_small_theta_rank``, one
  workgroup per run that keeps the run's normalised directions, then cls and val and the clusters' member lists in LDS
  (``tdea_small.hip``; the caps of ``rvea_small_select``).  Directions that are not batched stay shared.  Every output of run r is
  the 2-D op's on that run, bit for bit (``tests/test_batched_tdea_gpu.py``);
* ``bige_small_estimate_rank``: fit (B, n, m), mask (B, n), r (B,) → itself, one workgroup per run that keeps the run's normalised
  rows in LDS, forms the bi-goal estimate and ranks its points there (``bige_small.hip``; n ≤ 2048, 1024 or 512 for m ≤ 4, 8 or 16
  per run); ``ops.bige.estimate_rank`` calls it with a run's own operands under ``vmap``, and an unbatched operand is broadcast.
  Every output of run r is ``bige_estimate``'s and the non-dominated sort's on that run, bit for bit
  (``tests/test_batched_bige_gpu.py``).  ``bige_estimate`` has no batched form: its rule passes unbatched calls through and raises
  on batched operands;
* ``sra_select``: obj (B, n, m), u (B, n − 1), pc (B,) → ``sra_small_select``, one workgroup per run that forms both indicators and
  ranks the rows without writing the indicators to global memory in between (``sra_small.hip``; n ≤ 2048 at m ≤ 8, n ≤ 1024 at
  m ≤ 16 per run); an unbatched operand is broadcast.  Every output of run r is the 2-D op's on that run, bit for bit
  (``tests/test_batched_sra_gpu.py``).  ``sra_indicators`` and ``sra_rank`` have no batched form: their rules pass unbatched calls
  through and raise on batched operands.

Each run's words/trials are bit-identical to the single-run op with that run's key
(``tests/test_batched_runs.py``), each run's sorted keys and indices to the op applied row by row
(``tests/test_kernels_gpu.py``), each run's ranks, survivors and offspring to the single-run ops
(``tests/test_batched_mo_gpu.py``, ``tests/test_batched_ibea_spea2_gpu.py``, ``tests/test_batched_moead_gpu.py``, ``tests/test_nsga3_assoc_gpu.py``).  A per-run shape above a batched kernel's cap raises
``NotImplementedError``: there is no silent run-by-run fallback.  This mirrors the reference's use of ``jax.vmap`` for
independent copies of a workflow (``run/run_de.py:54-114`` runs 32 seeds per function).
"""
from __future__ import annotations

import torch

from . import _ext

_REGISTERED = False


def _front(x, bdim, B):
    """Run axis first (broadcast an unbatched operand), contiguous."""
    if bdim is None:
        return x.unsqueeze(0).expand((B,) + tuple(x.shape)).contiguous()
    return x.movedim(bdim, 0).contiguous()


def _philox_words(info, in_dims, key, nblocks, domain, offset, words=4):
    if in_dims[0] is None:
        return _ext.ops().philox_words(key, nblocks, domain, offset, words), None
    return _ext.ops().philox_words(_front(key, in_dims[0], info.batch_size), nblocks, domain, offset, words), 0


def _philox_fill(info, in_dims, key, n, dist, offset):
    if in_dims[0] is None:
        return _ext.ops().philox_fill(key, n, dist, offset), None
    return _ext.ops().philox_fill(_front(key, in_dims[0], info.batch_size), n, dist, offset), 0


def _rank_argsort_f32(info, in_dims, keys, descending):
    if in_dims[0] is None:
        return tuple(_ext.ops().rank_argsort_f32(keys, descending)), (None, None)
    k = _front(keys, in_dims[0], info.batch_size)
    if k.dim() != 2:
        raise NotImplementedError("rank_argsort_f32 vmap rule: per-run keys must be 1-D")
    ok, oi = _ext.ops().rank_argsort_f32(k, descending)
    return (ok, oi), (0, 0)


def _de_trial(info, in_dims, P, idx, coef, cur, mode, CR, jr, L, key, lb, ub, repair, err, col0=0, d_total=0):
    B = info.batch_size
    if any(d is not None for d in in_dims[9:11]) or in_dims[12] is not None:
        raise NotImplementedError("de_trial vmap rule: bounds and the error word must be shared by all runs")
    args = [_front(t, d, B) for t, d in zip((P, idx, coef, cur, mode, CR, jr, L, key), in_dims[:9])]
    return _ext.ops().de_trial(*args, lb, ub, repair, err, col0, d_total), 0


def _sbx(info, in_dims, x, keys, pro_c, dis_c, type, col0=0, dtot=0):
    if in_dims[0] is None and in_dims[1] is None:
        return _ext.ops().sbx(x, keys, pro_c, dis_c, type, col0, dtot), None
    B = info.batch_size
    xb = _front(x, in_dims[0], B)
    if xb.dim() != 3:
        raise NotImplementedError("sbx vmap rule: per-run x must be (n, d)")
    return _ext.ops().sbx(xb, _front(keys, in_dims[1], B), pro_c, dis_c, type, col0, dtot), 0


def _pm(info, in_dims, x, lb, ub, keys, pro_m, dis_m, nm, col0=0, dtot=0):
    if in_dims[1] is not None or in_dims[2] is not None:
        raise NotImplementedError("pm vmap rule: bounds must be shared by all runs")
    if in_dims[0] is None and in_dims[3] is None:
        return _ext.ops().pm(x, lb, ub, keys, pro_m, dis_m, nm, col0, dtot), None
    B = info.batch_size
    xb = _front(x, in_dims[0], B)
    if xb.dim() != 3:
        raise NotImplementedError("pm vmap rule: per-run x must be (n, d)")
    return _ext.ops().pm(xb, lb, ub, _front(keys, in_dims[3], B), pro_m, dis_m, nm, col0, dtot), 0


def _nds(info, in_dims, f, limit=0, err=None):
    from .nds import check_batched_caps

    # trailing arguments left at their schema defaults are not passed on, so in_dims can be shorter than the signature
    if len(in_dims) > 2 and in_dims[2] is not None:
        raise NotImplementedError("nds vmap rule: the error word must be shared by all runs")
    if in_dims[0] is None:
        return _ext.ops().nds(f, limit, err), None
    fb = _front(f, in_dims[0], info.batch_size)
    if fb.dim() != 3:
        raise NotImplementedError("nds vmap rule: per-run fitness must be (n, m)")
    check_batched_caps(fb.shape[1], fb.shape[2], "nds vmap rule")
    return _ext.ops().nds(fb, limit, None), 0  # one workgroup per run: no grid barrier, so no error path


def _nsga_select(info, in_dims, rank, f, N, mask_pos):
    from .nds import check_batched_caps

    if in_dims[0] is None and in_dims[1] is None:
        return _ext.ops().nsga_select(rank, f, N, mask_pos), None
    B = info.batch_size
    fb = _front(f, in_dims[1], B)
    if fb.dim() != 3:
        raise NotImplementedError("nsga_select vmap rule: per-run fitness must be (n, m)")
    check_batched_caps(fb.shape[1], 1, "nsga_select vmap rule")
    return _ext.ops().nsga_select(_front(rank, in_dims[0], B), fb, N, mask_pos), 0


def _runs_of(x, bdim, B, per_run_dim, what):
    """``_front`` of an operand whose per-run form has ``per_run_dim`` dimensions."""
    xb = _front(x, bdim, B)
    if xb.dim() != per_run_dim + 1:
        raise NotImplementedError(f"{what}: a per-run operand has {xb.dim() - 1} dimensions where {per_run_dim} are due")
    return xb


def _ibea_fitness(info, in_dims, obj, kappa):
    from .ibea import check_batched_caps

    ob = _runs_of(obj, in_dims[0], info.batch_size, 2, "ibea_fitness vmap rule")
    check_batched_caps(ob.shape[1], ob.shape[2], "ibea_fitness vmap rule", need_rows=False)
    return list(_ext.ops().ibea_fitness(ob, kappa)), [0, 0]


def _ibea_truncate(info, in_dims, obj, f, C, kappa, n_remove, n_keep):
    from .ibea import check_batched_caps

    B, what = info.batch_size, "ibea_truncate vmap rule"
    ob = _runs_of(obj, in_dims[0], B, 2, what)
    check_batched_caps(ob.shape[1], ob.shape[2], what)
    return list(_ext.ops().ibea_truncate(ob, _runs_of(f, in_dims[1], B, 1, what), _runs_of(C, in_dims[2], B, 1, what), kappa,
                                         n_remove, n_keep)), [0, 0]


def _spea2_fitness(info, in_dims, obj):
    from .spea2 import FIT_N_CAP, check_batched_caps

    ob = _runs_of(obj, in_dims[0], info.batch_size, 2, "spea2_fitness vmap rule")
    check_batched_caps(ob.shape[1], ob.shape[2], "spea2_fitness vmap rule", FIT_N_CAP)
    return list(_ext.ops().spea2_fitness(ob)), [0] * 8


def _spea2_truncate(info, in_dims, obj, mask, n_keep, nn_d2=None, nn_idx=None):
    from .spea2 import check_batched_caps

    B, what = info.batch_size, "spea2_truncate vmap rule"
    if (nn_d2 is None) != (nn_idx is None):
        raise NotImplementedError(f"{what}: nn_d2 and nn_idx are given together or not at all")
    ob = _runs_of(obj, in_dims[0], B, 2, what)
    check_batched_caps(ob.shape[1], ob.shape[2], what)
    if nn_d2 is not None:  # in_dims stops at the last argument that was passed
        nn_d2, nn_idx = _runs_of(nn_d2, in_dims[3], B, 1, what), _runs_of(nn_idx, in_dims[4], B, 1, what)
    return list(_ext.ops().spea2_truncate(ob, _runs_of(mask, in_dims[1], B, 1, what), n_keep, nn_d2, nn_idx)), [0, 0, 0]


def _cma_small_ask(info, in_dims, key, mean, sigma, B, D, lam):
    from .cma_small import check_batched_caps

    R, what = info.batch_size, "cma_small_ask vmap rule"
    mb = _runs_of(mean, in_dims[1], R, 1, what)
    check_batched_caps(mb.shape[1], lam, what)
    return _ext.ops().cma_small_ask(_runs_of(key, in_dims[0], R, 1, what), mb, _runs_of(sigma, in_dims[2], R, 0, what),
                                    _runs_of(B, in_dims[3], R, 2, what), _runs_of(D, in_dims[4], R, 1, what), lam), 0


def _cma_small_tell(info, in_dims, population, fitness, mean, sigma, ps, pc, C, B, D, invsqrtC, count_iter, count_eigen, weights, consts,
                    decomp_per_iter, eig_stats):
    from .cma_small import check_batched_caps

    R, what = info.batch_size, "cma_small_tell vmap rule"
    if in_dims[12] is not None:
        raise NotImplementedError(f"{what}: the recombination weights must be shared by all runs")
    pb = _runs_of(population, in_dims[0], R, 2, what)
    check_batched_caps(pb.shape[2], pb.shape[1], what)
    per_run = ((fitness, 1), (mean, 1), (sigma, 0), (ps, 1), (pc, 1), (C, 2), (B, 2), (D, 1), (invsqrtC, 2), (count_iter, 0), (count_eigen, 0))
    args = [_runs_of(t, bd, R, nd, what) for (t, nd), bd in zip(per_run, in_dims[1:12])]
    out = _ext.ops().cma_small_tell(pb, *args, weights, consts, decomp_per_iter, _runs_of(eig_stats, in_dims[15], R, 1, what))
    return list(out), [0] * 10


def _shared_or_runs(x, bdim, B, per_run_dim, what):
    """An operand the runs may share: (1, …) where unbatched or broadcast along the run axis (what ``vmap`` makes of a
    constant that a vmapped ``init`` returned), ``_runs_of`` otherwise.  The stride test is an optimisation only: once a workflow
    or a graph has cloned the state, the same table arrives R times and takes the per-run path, with the same bits
    (``tests/test_batched_moead_gpu.py`` holds the shared, the broadcast and the per-run form to each other)."""
    if bdim is None:
        return x.unsqueeze(0).contiguous()
    xb = x.movedim(bdim, 0)
    if xb.stride(0) == 0 and xb.dim() == per_run_dim + 1:
        return xb[:1].contiguous()
    return _runs_of(x, bdim, B, per_run_dim, what)


def _moead_small_ask(info, in_dims, pop, nb, key, kx, km, lb, ub, pro_c, dis_c, pro_m, dis_m, nm):
    R, what = info.batch_size, "moead_small_ask vmap rule"
    if in_dims[5] is not None or in_dims[6] is not None:
        raise NotImplementedError(f"{what}: bounds must be shared by all runs")
    out = _ext.ops().moead_small_ask(_runs_of(pop, in_dims[0], R, 2, what), _shared_or_runs(nb, in_dims[1], R, 2, what),
                                     _runs_of(key, in_dims[2], R, 1, what), _runs_of(kx, in_dims[3], R, 2, what),
                                     _runs_of(km, in_dims[4], R, 2, what), lb, ub, pro_c, dis_c, pro_m, dis_m, nm)
    return list(out), [0, 0]


def _moead_small_tell(info, in_dims, pop, off, pop_obj, off_obj, W, nb, z, func):
    from .mo import check_small_caps

    R, what = info.batch_size, "moead_small_tell vmap rule"
    ob = _runs_of(off_obj, in_dims[3], R, 2, what)
    check_small_caps(ob.shape[1], ob.shape[2], what)
    out = _ext.ops().moead_small_tell(_runs_of(pop, in_dims[0], R, 2, what), _runs_of(off, in_dims[1], R, 2, what),
                                      _runs_of(pop_obj, in_dims[2], R, 2, what), ob, _shared_or_runs(W, in_dims[4], R, 2, what),
                                      _shared_or_runs(nb, in_dims[5], R, 2, what), _runs_of(z, in_dims[6], R, 1, what), func)
    return list(out), [0, 0, 0, 0]


def _nsga3_associate(info, in_dims, f, rank, ref, N):
    from .nsga3 import check_batched_caps

    B, what = info.batch_size, "nsga3_associate vmap rule"
    if in_dims[2] is not None:
        raise NotImplementedError(f"{what}: the reference points must be shared by all runs")
    fb = _runs_of(f, in_dims[0], B, 2, what)
    check_batched_caps(fb.shape[1], fb.shape[2], ref.shape[0], what)
    return list(_ext.ops().nsga3_associate(fb, _runs_of(rank, in_dims[1], B, 1, what), ref, N)), [0, 0, 0, 0]


def _nsga3_niche_select(info, in_dims, rank, last_rank, group, group_dist, key, N, R):
    from .nds import NICHE_SELECT_CAP

    B, what = info.batch_size, "nsga3_niche_select vmap rule"
    rb = _runs_of(rank, in_dims[0], B, 1, what)
    if rb.shape[1] > NICHE_SELECT_CAP or R > NICHE_SELECT_CAP:
        raise NotImplementedError(f"{what}: batched runs need n <= {NICHE_SELECT_CAP} rows and R <= {NICHE_SELECT_CAP} reference "
                                  f"points per run, got n = {rb.shape[1]}, R = {R}")
    return _ext.ops().nsga3_niche_select(rb, _runs_of(last_rank, in_dims[1], B, 0, what), _runs_of(group, in_dims[2], B, 1, what),
                                         _runs_of(group_dist, in_dims[3], B, 1, what), _runs_of(key, in_dims[4], B, 1, what), N, R), 0


def _hype_fitness(info, in_dims, points, ref, alpha, key, n_sample):
    from .geom import hype_fused_ok

    B, what = info.batch_size, "hype_fitness vmap rule"
    if in_dims[2] is not None:
        raise NotImplementedError(f"{what}: alpha must be shared by all runs")
    if in_dims[0] is None and in_dims[1] is None and in_dims[3] is None:
        return _ext.ops().hype_fitness(points, ref, alpha, key, n_sample), None
    pb = _runs_of(points, in_dims[0], B, 2, what)
    if not hype_fused_ok(pb.shape[1], pb.shape[2], n_sample):
        raise NotImplementedError(f"{what}: batched runs need n <= 2048, m <= 16 and n_sample <= 2^20 per run, got n = {pb.shape[1]}, "
                                  f"m = {pb.shape[2]}, n_sample = {n_sample}")
    return _ext.ops().hype_fitness(pb, _runs_of(ref, in_dims[1], B, 1, what), alpha, _runs_of(key, in_dims[3], B, 1, what), n_sample), 0


def _hv_count(info, in_dims, S, P, strict):
    if in_dims[0] is not None or in_dims[1] is not None:
        raise NotImplementedError("hv_count vmap rule: no batched form (HypE's batched runs go through hype_fitness, within its caps)")
    return _ext.ops().hv_count(S, P, strict), None


def _hv_contrib(info, in_dims, S, P, count, alpha):
    if any(d is not None for d in in_dims):
        raise NotImplementedError("hv_contrib vmap rule: no batched form (HypE's batched runs go through hype_fitness, within its caps)")
    return _ext.ops().hv_contrib(S, P, count, alpha), None


def _rvea_select(info, in_dims, f, shift, floor, v, theta):
    from .rvea import check_small_caps

    B, what = info.batch_size, "rvea_select vmap rule"
    if all(d is None for d in in_dims):
        return list(_ext.ops().rvea_select(f, shift, floor, v, theta)), [None] * 5
    if shift is None or floor is None:
        raise NotImplementedError(f"{what}: batched runs take a shift and a floor (the APD selection passes both)")
    fb = _runs_of(f, in_dims[0], B, 2, what)
    vb = _runs_of(v, in_dims[3], B, 2, what)
    check_small_caps(fb.shape[1], vb.shape[1], fb.shape[2], what)
    out = _ext.ops().rvea_small_select(fb, _runs_of(shift, in_dims[1], B, 1, what), floor, vb, _front(theta, in_dims[4], B).reshape(B))
    return list(out), [0] * 5


def _rvea_cos_best(info, in_dims, A, shift, floor, B, clamp, self_zero):
    if any(d is not None for d in in_dims):
        raise NotImplementedError("rvea_cos_best vmap rule: no batched form (RVEA's batched runs go through rvea_select and θ-DEA's "
                                  "through tdea_theta_rank, within their caps; RVEA* and LMOCSO are not covered)")
    return list(_ext.ops().rvea_cos_best(A, shift, floor, B, clamp, self_zero)), [None, None]


def _tdea_theta_rank(info, in_dims, obj, w, theta, mask):
    from .rvea import check_small_caps

    B, what = info.batch_size, "tdea_theta_rank vmap rule"
    if all(d is None for d in in_dims):
        return list(_ext.ops().tdea_theta_rank(obj, w, theta, mask)), [None] * 3
    ob = _runs_of(obj, in_dims[0], B, 2, what)
    wb = w if in_dims[1] is None else _runs_of(w, in_dims[1], B, 2, what)  # directions the runs share stay (nw, m)
    tb = theta if in_dims[2] is None else _runs_of(theta, in_dims[2], B, 1, what)
    check_small_caps(ob.shape[1], wb.shape[-2], ob.shape[2], what)
    return list(_ext.ops().tdea_small_theta_rank(ob, wb, tb, _runs_of(mask, in_dims[3], B, 1, what))), [0, 0, 0]


def _bige_small_estimate_rank(info, in_dims, fit, mask, r):
    from .bige import check_small_caps

    B, what = info.batch_size, "bige_small_estimate_rank vmap rule"
    fb = _runs_of(fit, in_dims[0], B, 2, what)
    check_small_caps(fb.shape[1], fb.shape[2], what)
    out = _ext.ops().bige_small_estimate_rank(fb, _runs_of(mask, in_dims[1], B, 1, what), _front(r, in_dims[2], B).reshape(B))
    return list(out), [0] * 4


def _bige_estimate(info, in_dims, fit, mask, r):
    if any(d is not None for d in in_dims):
        raise NotImplementedError("bige_estimate vmap rule: no batched form (BiGE's batched runs go through bige_small_estimate_rank, "
                                  "within its caps)")
    return list(_ext.ops().bige_estimate(fit, mask, r)), [None] * 3


def _sra_select(info, in_dims, obj, u, pc):
    from .sra import check_small_caps

    B, what = info.batch_size, "sra_select vmap rule"
    if all(d is None for d in in_dims):
        return list(_ext.ops().sra_select(obj, u, pc)), [None] * 3
    ob = _runs_of(obj, in_dims[0], B, 2, what)
    check_small_caps(ob.shape[1], ob.shape[2], what)
    out = _ext.ops().sra_small_select(ob, _runs_of(u, in_dims[1], B, 1, what), _front(pc, in_dims[2], B).reshape(B))
    return list(out), [0] * 3


def _sra_indicators(info, in_dims, obj):
    if in_dims[0] is not None:
        raise NotImplementedError("sra_indicators vmap rule: no batched form (SRA's batched runs go through sra_select, within its caps)")
    return list(_ext.ops().sra_indicators(obj)), [None, None]


def _sra_rank(info, in_dims, I1, I2, u, pc):
    if any(d is not None for d in in_dims):
        raise NotImplementedError("sra_rank vmap rule: no batched form (SRA's batched runs go through sra_select, within its caps)")
    return _ext.ops().sra_rank(I1, I2, u, pc), None


def register():
    """Install the rules (idempotent).  Without the compiled extension there is nothing to
    batch: CPU tensors never reach the HIP ops, and a device op raises on its own."""
    global _REGISTERED
    if _REGISTERED or not _ext.load(build_if_missing=False):
        return
    for name, fn in (("philox_words", _philox_words), ("philox_fill", _philox_fill), ("rank_argsort_f32", _rank_argsort_f32),
                     ("de_trial", _de_trial), ("sbx", _sbx), ("pm", _pm), ("nds", _nds), ("nsga_select", _nsga_select),
                     ("ibea_fitness", _ibea_fitness), ("ibea_truncate", _ibea_truncate), ("spea2_fitness", _spea2_fitness),
                     ("spea2_truncate", _spea2_truncate), ("cma_small_ask", _cma_small_ask), ("cma_small_tell", _cma_small_tell),
                     ("moead_small_ask", _moead_small_ask), ("moead_small_tell", _moead_small_tell),
                     ("nsga3_associate", _nsga3_associate), ("nsga3_niche_select", _nsga3_niche_select),
                     ("hype_fitness", _hype_fitness), ("hv_count", _hv_count), ("hv_contrib", _hv_contrib),
                     ("rvea_select", _rvea_select), ("rvea_cos_best", _rvea_cos_best), ("tdea_theta_rank", _tdea_theta_rank),
                     ("bige_small_estimate_rank", _bige_small_estimate_rank), ("bige_estimate", _bige_estimate),
                     ("sra_select", _sra_select), ("sra_indicators", _sra_indicators), ("sra_rank", _sra_rank)):
        torch.library.register_vmap(f"evoxmi::{name}", fn)
    _REGISTERED = True
