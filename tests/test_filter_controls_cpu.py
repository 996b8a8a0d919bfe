"""The inputs of tests/test_gpu_filter_controls.py on the CPU: the pictures hold the boundary-strength cases and the filter activity the GPU
cases assert, counted with the oracle's boundary strengths (tests/bs_ref.py checks its own restatement against them unit by unit)."""
import pytest

from tests import test_gpu_filter_controls as gpu_cases


@pytest.mark.parametrize("bi", [False, True])
@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_motion_pictures_hold_every_boundary_strength_case(oracle, fmt, bi):
    p, ref0, ref1, cur = gpu_cases.motion_picture(fmt, bi)
    want = gpu_cases.oracle_chain(oracle, p, cur, [ref0, ref1])
    counts, changed = gpu_cases.check_content(oracle, p, want, bi)
    assert (counts["swapped lists"] > 0) == bi
    m = p.meta_np
    assert ((m["ref_idx1"] == 1).any() and len({int(p.slice.ref_pic[1][i]) for i in range(2)}) == 2) == bi
