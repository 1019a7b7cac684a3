"""``CMAES(fused_small=True)`` on CPU tensors: the flag is accepted and the torch path runs unchanged."""
import torch

from evoxmi import random as rnd
from evoxmi.algorithms import CMAES


def test_fused_small_on_cpu_is_the_torch_path():
    def run(flag):
        a = CMAES(torch.full((10,), 3.0), 1.0, fused_small=flag)
        st = a.init(rnd.PRNGKey(7))
        for _ in range(5):
            pop, st = a.ask(st)
            st = a.tell(st, (pop * pop).sum(1))
        return st

    s0, s1 = run(False), run(True)
    assert set(s0._state_dict) == set(s1._state_dict)
    for name, v in s0._state_dict.items():
        assert torch.equal(v, s1[name]), name
