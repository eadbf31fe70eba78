"""CPU-only: the compiled output-masking kernel (k_mask_rows, blind issuance) needs no scratch and no LDS.  Reads the metadata of the
gfx950 code object of the built library - private_segment_fixed_size and group_segment_fixed_size, nothing else - through the fixture
of tests/test_kernel_isa.py."""
from tests.test_kernel_isa import code_object  # noqa: F401 (the module fixture)


def test_k_mask_rows_uses_no_scratch_and_no_lds(code_object):  # noqa: F811
    kernels, _ = code_object
    names = [k for k in kernels if k.startswith("_Z11k_mask_rowsP")]
    assert len(names) == 1, sorted(kernels)
    k = kernels[names[0]]
    assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, (names[0], k)
