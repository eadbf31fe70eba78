"""CPU-only: the two kernels of the batchable verification's coefficient stage (aeonflux_amd/csrc/batchable.cuh) in the built gfx950
code object: no scratch and no LDS - the Keccak state of k_batch_weights and the accumulators of k_coef stay in registers - and
registers that leave several blocks resident.  Reads the code object of the built library, as tests/test_kernel_isa.py does (which
still sees ONE gfx950 code object: the kernels are part of the library's single device translation unit)."""
from tests.test_kernel_isa import code_object  # noqa: F401 (the module fixture)


def _one(kernels, prefix):
    name = [k for k in kernels if k.startswith(prefix)]
    assert len(name) == 1, sorted(kernels)
    return name[0]


def test_k_coef_and_k_batch_weights_use_no_scratch_and_no_lds(code_object):  # noqa: F811
    kernels, bodies = code_object
    for prefix in ("_Z6k_coef", "_Z15k_batch_weights"):
        name = _one(kernels, prefix)
        k = kernels[name]
        assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, (name, k)
        body = bodies[name]
        assert "scratch_" not in body and "ds_" not in body, name
        assert k["vgpr_count"] <= 128, (name, k)   # four blocks of 256 per compute unit
    # the figures DESIGN.md section 3 quotes for the two kernels
    assert kernels[_one(kernels, "_Z15k_batch_weights")]["vgpr_count"] <= 81 and kernels[_one(kernels, "_Z6k_coef")]["vgpr_count"] <= 92


def test_k_coef_reads_its_triples_with_scalar_loads(code_object):  # noqa: F811
    kernels, bodies = code_object
    body = bodies[_one(kernels, "_Z6k_coef")]
    assert "s_load_dword" in body          # the job and its wave-uniform triples
    assert "global_store_dwordx4" in body or "flat_store_dwordx4" in body   # the output scalar: two 16-byte stores
