"""The decisions of every case of tests/test_gpu_fqf.py, from the models alone (no GPU): a seed that puts an a* tie or a relu sign within
Float32 rounding shows up here.

a*          the float64 model's top-two gap of Q(s') is >= 100 x the Q floor of the case's bar x max|theta|, on its own fractions and
            teacher-forced on the Float32 model's levels; the float64 and the Float32 model choose the same a* everywhere.
relu signs  the float64 model's smallest |pre-activation| (psi where act is relu, phi always, of every network evaluation in the loss)
            is >= 100 x the largest distance of a Float32 pre-activation from its float64 one, both models on the same levels.
carry       the carry cases hold more tiles than dist_num_blocks hands out workgroups (the rule restated: min(256, 16 MiB of rows))."""
import numpy as np
import pytest

import test_gpu_fqf as G


@pytest.mark.parametrize("name", list(G.CASES))
def test_no_case_decides_within_float32_rounding(name):
    fl, own, dec = G.floors(name)
    q_floor = G.bars(name)[0]["q"]
    print(f"fqf {name}: a* margin {dec['margin']:.2e} (needs {100 * q_floor * dec['thmax']:.2e}), zmin {dec['zmin']:.2e} (needs {100 * dec['zdist']:.2e}); "
          "floors " + ", ".join(f"{k} {v:.2e}" for k, v in fl.items()))
    assert dec["margin"] >= 100 * q_floor * dec["thmax"], f"{name}: a* margin {dec['margin']:.1e}; choose another seed"
    assert dec["zmin"] >= 100 * dec["zdist"], f"{name}: a pre-activation is {dec['zmin']:.1e} from zero; choose another seed"
    s32, s64, sown = dec["sel"]
    assert np.array_equal(s32, s64) and np.array_equal(s64, sown), f"{name}: the float64 and the Float32 model choose different a*"


@pytest.mark.parametrize("name", G.CARRY)
def test_carry_cases_exceed_the_workgroup_count(name):
    c = G.case(name)
    ns, h, na, nc = c["dims"]
    row = h * ns + h + h * nc + h + na * h + na + c["N"] * h + c["N"]
    assert 8 * min(256, (16 << 20) // (4 * row)) < c["b"]
