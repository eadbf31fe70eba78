"""CPU-only: the two kernels of the presentation tags (aeonflux_amd/csrc/tags.cuh) in the built gfx950 code object.  k_sc_invert - the
one kernel that handles the secret-derived s = m + n - keeps its operands and the 512-bit product in registers: no scratch, no LDS
(a table of powers indexed by a run-time digit would have gone to scratch), a ROLLED loop over the bits of the public exponent (a few
branches, not 324 inlined products), and its only memory accesses are the loads of its two operands, the stores of its row and the
scalar loads of constants.  Reads the code object of the built library, as tests/test_kernel_isa.py does."""
import re

from tests.test_kernel_isa import code_object  # noqa: F401 (the module fixture)


def _one(kernels, prefix):
    name = [k for k in kernels if k.startswith(prefix)]
    assert len(name) == 1, sorted(kernels)
    return name[0]


def test_k_sc_invert_uses_no_scratch_and_no_lds(code_object):  # noqa: F811
    kernels, bodies = code_object
    for prefix in ("_Z11k_sc_invert", "_Z15k_tag_broadcast"):
        name = _one(kernels, prefix)
        k = kernels[name]
        assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, (name, k)
        body = bodies[name]
        assert "scratch_" not in body and "ds_" not in body, name
    # measured at build time: 76 VGPRs (six blocks of 256 per compute unit); DESIGN.md quotes the figure
    assert kernels[_one(kernels, "_Z11k_sc_invert")]["vgpr_count"] <= 76, kernels[_one(kernels, "_Z11k_sc_invert")]


def test_k_sc_invert_is_a_rolled_loop_with_operand_independent_addresses(code_object):  # noqa: F811
    kernels, bodies = code_object
    body = bodies[_one(kernels, "_Z11k_sc_invert")]
    # two inlined products (the squaring and the multiplication by the base): 2 x 64 multiply-adds of mp_mul<8, 8> and the folds of two
    # reductions - a few hundred, where 324 inlined products would be tens of thousands
    assert 128 <= len(re.findall(r"\bv_mad_u64_u32\b", body)) <= 600, len(re.findall(r"\bv_mad_u64_u32\b", body))
    assert len(re.findall(r"\bs_cbranch_\w+", body)) <= 6
    # vector memory: the operands in (2 x 32 bytes), the row out (2 x 16 bytes), nothing inside the loop
    loads = re.findall(r"\b(?:global|flat)_load_\w+", body)
    stores = re.findall(r"\b(?:global|flat)_store_\w+", body)
    assert 1 <= len(loads) <= 16 and 1 <= len(stores) <= 2, (loads, stores)
    assert all(s.endswith("dwordx4") for s in stores), stores
    assert "buffer_" not in body
