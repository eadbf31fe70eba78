"""CPU-only: the four kernels of the whole-message calls (aeonflux_amd/csrc/messages.cuh) - the chunk gather, the key-row expansion, the
per-message status and masking, the candidate at a known counter - use no scratch and no LDS, and k_encode_at, which is
k_encode_to_group without its loop, needs no more private memory or vector registers than k_decode, whose decoding it runs.  Reads the
gfx950 code object of the built library, as tests/test_kernel_isa.py does."""
from tests.test_kernel_isa import code_object  # noqa: F401 (the module fixture)

NEW = ("k_msg_gather", "k_msg_expand", "k_msg_status", "k_encode_at")


def _one(kernels, stem):
    names = [k for k in kernels if k.startswith("_Z%d%s" % (len(stem), stem))]
    assert len(names) == 1, (stem, sorted(kernels))
    return names[0]


def test_the_message_kernels_use_no_scratch_and_no_lds(code_object):  # noqa: F811
    kernels, bodies = code_object
    for stem in NEW:
        name = _one(kernels, stem)
        k = kernels[name]
        assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, (name, k)
        body = bodies[name]
        assert "scratch_" not in body and "ds_" not in body, name


def test_the_gather_expansion_and_status_kernels_use_no_atomics(code_object):  # noqa: F811
    kernels, bodies = code_object
    for stem in NEW[:3]:
        assert "atomic" not in bodies[_one(kernels, stem)], stem


def test_k_encode_at_needs_no_more_than_k_decode(code_object):  # noqa: F811
    kernels, _ = code_object
    at, dec = kernels[_one(kernels, "k_encode_at")], kernels[_one(kernels, "k_decode")]   # (k_decode_mixed has another length prefix)
    print("k_encode_at", at, "k_decode", dec)
    assert at["private_segment_fixed_size"] <= dec["private_segment_fixed_size"], (at, dec)
    assert at["vgpr_count"] <= dec["vgpr_count"], (at, dec)
