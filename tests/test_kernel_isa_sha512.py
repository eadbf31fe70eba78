"""CPU-only: the compiled k_sha512 keeps its eight state words and its message schedule in registers - no scratch, no LDS - and
k_encode_to_group, whose loop runs the decoding k_decode runs, needs no more private memory than that kernel.  Reads the gfx950
code object of the built library, as tests/test_kernel_isa.py does."""
from tests.test_kernel_isa import code_object  # noqa: F401 (the module fixture)


def test_k_sha512_uses_no_scratch_and_no_lds(code_object):  # noqa: F811
    kernels, bodies = code_object
    names = [k for k in kernels if k.startswith("_Z8k_sha512P") or k.startswith("_Z15k_sha512_direct")]
    assert len(names) == 2, sorted(kernels)
    for name in names:
        k = kernels[name]
        assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, (name, k)
        body = bodies[name]
        assert "scratch_" not in body and "ds_" not in body, name


def test_k_encode_to_group_needs_no_more_private_memory_than_k_decode(code_object):  # noqa: F811
    kernels, _ = code_object
    enc = [k for k in kernels if k.startswith("_Z17k_encode_to_group")]
    dec = [k for k in kernels if k.startswith("_Z8k_decodeP")]
    assert len(enc) == 1 and len(dec) == 1, sorted(kernels)
    assert kernels[enc[0]]["private_segment_fixed_size"] <= kernels[dec[0]]["private_segment_fixed_size"], (kernels[enc[0]], kernels[dec[0]])
    assert kernels[enc[0]]["group_segment_fixed_size"] == 0
