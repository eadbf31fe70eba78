"""CPU-only: the compiled k_draw (device randomness, include/aeonflux_gpu.h afx_device_rng) keeps its Keccak state in registers - no
scratch, no LDS - and stores its draws with 16-byte vector stores.  Reads the gfx950 code object of the built library, as
tests/test_kernel_isa.py does."""
import re

from tests.test_kernel_isa import code_object  # noqa: F401 (the module fixture)


def test_k_draw_uses_no_scratch_and_no_lds(code_object):  # noqa: F811
    kernels, bodies = code_object
    name = [k for k in kernels if k.startswith("_Z6k_draw")]
    assert len(name) == 1, sorted(kernels)
    k = kernels[name[0]]
    assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, k
    body = bodies[name[0]]
    assert "scratch_" not in body and "buffer_store" not in body and "ds_" not in body
    assert len(re.findall(r"(flat|global)_store_dwordx4", body)) == 4, body   # (two for a 32-byte draw, two more for a 64-byte one)
