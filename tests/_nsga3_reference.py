"""Host reference of NSGA-III's normalisation and association (``evoxmi/ops/nsga3.py``), shared by test_batched_nsga3.py and
test_nsga3_assoc_gpu.py.  Plain numpy float64; the ranks are an input.  The perpendicular distance is the norm of the rejection
x − (x·ŵ)ŵ, which has no cancellation."""
import numpy as np


def associate(f, rank, ref, N, chunk=512):
    """dict: last_rank, ideal, extreme (m rows), cond (of the extreme system; inf when an extreme row repeats), worst, nadir, used_worst,
    xnorm (n,), dmin (n,) every row's smallest distance, and dist_to(group) → the distance of every row to ref[group[row]]."""
    f, ref = np.asarray(f, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rank = np.asarray(rank)
    n, m = f.shape
    last_rank = np.sort(rank, kind="stable")[N]
    valid = rank <= last_rank
    ideal = f[valid].min(0)
    Fn = f - ideal
    asf = (Fn[None, :, :] / (np.eye(m) + 1e-6)[:, None, :]).max(-1)  # (m, n)
    asf[:, ~valid] = np.inf
    extreme = asf.argmin(1)
    worst = Fn[valid].max(0)
    E = Fn[extreme]
    ok, cond, nadir = len(set(extreme.tolist())) == m, np.inf, worst  # a repeated extreme row: singular
    try:
        if ok:
            cond, intercept = float(np.linalg.cond(E)), 1.0 / np.linalg.solve(E, np.ones(m))
            ok = bool(np.isfinite(intercept).all() and (intercept > 1e-6).all())
    except np.linalg.LinAlgError:
        ok = False
    nadir = intercept if ok else worst
    x = Fn / nadir
    what = ref / np.linalg.norm(ref, axis=1, keepdims=True)

    def dist_to(group):  # every row against its own reference point
        w = what[np.asarray(group)]
        return np.linalg.norm(x - (x * w).sum(1, keepdims=True) * w, axis=1)

    def dmin_of(xs):  # a chunk of rows against every reference point
        return np.linalg.norm(xs[:, None, :] - (xs @ what.T)[:, :, None] * what[None, :, :], axis=2).min(1)

    dmin = np.concatenate([dmin_of(x[i:i + chunk]) for i in range(0, n, chunk)])
    return dict(last_rank=int(last_rank), ideal=ideal, extreme=extreme, cond=cond, worst=worst, nadir=nadir, used_worst=not ok,
                xnorm=np.linalg.norm(x, axis=1), dmin=dmin, dist_to=dist_to)
