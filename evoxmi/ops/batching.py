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
  is the single-run one (n ≤ 8192, m ≤ 16 per run); SPEA2's runs each count their own removals.

Each run's words/trials are bit-identical to the single-run op with that run's key
(``tests/test_batched_runs.py``), each run's sorted keys and indices to the op applied row by row
(``tests/test_kernels_gpu.py``), each run's ranks, survivors and offspring to the single-run ops
(``tests/test_batched_mo_gpu.py``, ``tests/test_batched_ibea_spea2_gpu.py``).  A per-run shape above a batched kernel's cap raises
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


def register():
    """Install the rules (idempotent).  Without the compiled extension there is nothing to
    batch: CPU tensors never reach the HIP ops, and a device op raises on its own."""
    global _REGISTERED
    if _REGISTERED or not _ext.load(build_if_missing=False):
        return
    for name, fn in (("philox_words", _philox_words), ("philox_fill", _philox_fill), ("rank_argsort_f32", _rank_argsort_f32),
                     ("de_trial", _de_trial), ("sbx", _sbx), ("pm", _pm), ("nds", _nds), ("nsga_select", _nsga_select),
                     ("ibea_fitness", _ibea_fitness), ("ibea_truncate", _ibea_truncate), ("spea2_fitness", _spea2_fitness),
                     ("spea2_truncate", _spea2_truncate)):
        torch.library.register_vmap(f"evoxmi::{name}", fn)
    _REGISTERED = True
