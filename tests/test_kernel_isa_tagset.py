"""CPU-only: the three kernels of the spent-tag set (aeonflux_amd/csrc/tagset.cuh) in the built gfx950 code object.  They exist, keep the
sponge of the slot function in registers (no scratch, no LDS), and talk to each other through the atomics the header names and nothing
else: one compare-and-swap and one unsigned minimum in k_tagset_claim, none in k_tagset_contains, one 64-bit add (the size, per wave)
in k_tagset_resolve; and no kernel waits (no s_sleep: there is no spin loop to put one in).  Reads the code object of the built
library, as tests/test_kernel_isa.py does."""
import re

from tests.test_kernel_isa import code_object  # noqa: F401 (the module fixture)

CLAIM, RESOLVE, CONTAINS = "_Z14k_tagset_claim", "_Z16k_tagset_resolve", "_Z17k_tagset_contains"


def _one(kernels, prefix):
    name = [k for k in kernels if k.startswith(prefix)]
    assert len(name) == 1, sorted(kernels)
    return name[0]


def test_the_three_kernels_exist_and_use_no_scratch_and_no_lds(code_object):  # noqa: F811
    kernels, bodies = code_object
    for prefix in (CLAIM, RESOLVE, CONTAINS):
        name = _one(kernels, prefix)
        k = kernels[name]
        assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, (name, k)
        body = bodies[name]
        assert "scratch_" not in body and not re.search(r"\bds_", body) and "buffer_" not in body, name
        assert "s_sleep" not in body, name
    # measured at build time: 79, 18 and 80 VGPRs (DESIGN.md quotes the figures): six blocks of 256 per compute unit at 80
    assert kernels[_one(kernels, CLAIM)]["vgpr_count"] <= 84, kernels[_one(kernels, CLAIM)]
    assert kernels[_one(kernels, CONTAINS)]["vgpr_count"] <= 84, kernels[_one(kernels, CONTAINS)]
    assert kernels[_one(kernels, RESOLVE)]["vgpr_count"] <= 32, kernels[_one(kernels, RESOLVE)]


def test_lanes_meet_only_in_the_atomics_the_header_names(code_object):  # noqa: F811
    kernels, bodies = code_object
    atomics = lambda prefix: sorted(re.findall(r"\b(?:global|flat)_atomic_\w+", bodies[_one(kernels, prefix)]))
    claim = atomics(CLAIM)
    assert [a for a in claim if "cmpswap" in a] == ["global_atomic_cmpswap"], claim           # owner
    assert [a for a in claim if "umin" in a] and all("cmpswap" in a or "umin" in a or "_or" in a for a in claim), claim   # lowest; the error word
    assert all("_or" in a for a in atomics(CONTAINS)), atomics(CONTAINS)                       # the error word alone: a lookup changes nothing
    assert atomics(RESOLVE) == ["global_atomic_add_x2"], atomics(RESOLVE)                      # the size, one add per wave
    # the lookup stores its answer byte and nothing else
    stores = re.findall(r"\b(?:global|flat)_store_\w+", bodies[_one(kernels, CONTAINS)])
    assert stores == ["global_store_byte"], stores
    # a claim stores slot_of[item] and nothing else: keys are written by the resolve launch, for LATER launches to read
    stores = re.findall(r"\b(?:global|flat)_store_\w+", bodies[_one(kernels, CLAIM)])
    assert stores and all(s == "global_store_dword" for s in stores), stores
