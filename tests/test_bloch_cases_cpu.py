"""The inputs of tests/test_bloch_gpu.py's steady-state cases are well-conditioned: with the oracle alone, no (frequency, position)
of any case has I - A within 1e-9 of singular, so the 1e-12 bound of the device against the oracle is meaningful there."""
import importlib.util
import os


def test_steady_state_cases_of_the_single_bloch_test_are_well_conditioned():
    spec = importlib.util.spec_from_file_location("bloch_gpu", os.path.join(os.path.dirname(__file__), "test_bloch_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cases = [c for c in mod.bloch_cases() if c[0] & 1]
    assert len(cases) == 9 + 6
    worst = min(mod.steady_state_margin(*mod.bloch_case(*c)[:7]) for c in cases)
    print("smallest singular value of I - A over the cases: %.3g" % worst)
    assert worst > 1e-9
