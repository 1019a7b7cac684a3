"""``BatchedRuns(HypE)`` on the device (MI355X, marked gpu): every run equals the solo workflow bit for bit, eager and captured in a
hipGraph, with functorch's run-by-run fallback switched off, so an op without a vmap rule raises.  Before ``hype_fitness.hip`` the batched
step ran ``hv_count`` and ``hv_contrib`` once per run through that fallback (``profiles/NOTES.md``)."""
import pytest
import torch

from test_batched_hype import check_runs_equal_solo

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_batched_hype_runs_equal_solo_gpu(graph):
    from evoxmi.ops import _ext

    assert _ext.load(), f"evoxmi extension must load on a GPU box: {_ext._ERROR!r}"
    was = torch._C._functorch._is_vmap_fallback_enabled()
    torch._C._functorch._set_vmap_fallback_enabled(False)
    try:
        check_runs_equal_solo("cuda", graph)
    finally:
        torch._C._functorch._set_vmap_fallback_enabled(was)
    _ext.check_kernel_errors()
