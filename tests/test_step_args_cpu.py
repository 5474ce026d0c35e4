"""Argument segment and scalar-register spills of the step kernels, read on the
CPU from the in-tree liblnw.so's gfx950 code object metadata (llvm-objcopy, the
offload bundler, llvm-readelf --notes), as test_kernel_resources_cpu.py reads
the scratch sizes.

The step kernels take their constants and array pointers by value. Before the
cold block (KCold, lnw_device.h) the segment was 1 128 B for every
instantiation, and the compiler fetched it in 16-dword pieces it could not
keep: 286 spilled scalar registers in the headline kernel, 346 (and 28 B per
lane of scratch) in the small-shard kernel. With the analytics channels, work
counters, tape RNG, spawn spec and bearing scratch behind one pointer the
segment is 992 B, and every instantiation spills less than it did. The bounds
below are the parent's figures (never to be reached again) and what this
layout reached (so that growth shows up here).
"""
import pytest

from _codeobj import LIB, kernel_metadata, needs_lib, needs_tools

pytestmark = [needs_lib, needs_tools]

PARENT_KERNARG = 1128
REACHED_KERNARG = 992

# template arguments <NB, NR, CW, REFW, UN, PS, SL> as mangled ->
#   (the parent's spilled SGPRs, what this layout reached, must be strictly below the parent's)
STEP_KERNELS = {
    "ILi4ELi4ELb0ELb0ELi4ELb0ELb0EE": (286, 169, True),    # headline: units kernel
    "ILi4ELi4ELb0ELb0ELi1ELb0ELb0EE": (346, 237, True),    # small shards
    "ILi4ELi4ELb0ELb0ELi1ELb0ELb1EE": (365, 255, False),   # two-slab direct rows
    "ILi4ELi4ELb1ELb0ELi1ELb0ELb0EE": (361, 282, False),   # contact variant (melee)
    "ILi4ELi4ELb1ELb0ELi1ELb1ELb0EE": (625, 434, False),   # contact, phase S by side
    "ILi3ELi3ELb0ELb0ELi1ELb0ELb0EE": (225, 186, False),
    "ILi3ELi3ELb1ELb0ELi1ELb0ELb0EE": (351, 266, False),
    "ILi2ELi2ELb0ELb0ELi1ELb0ELb0EE": (222, 189, False),
    "ILi2ELi2ELb1ELb0ELi1ELb0ELb0EE": (327, 261, False),
    "ILi0ELi0ELb0ELb0ELi1ELb0ELb0EE": (306, 271, False),   # runtime team sizes
    "ILi0ELi0ELb0ELb1ELi1ELb0ELb0EE": (317, 266, False),   # ... with the reference's LOS work
}
# the existing scratch limits of the two kernels the gain is judged on
SCRATCH_LIMIT = {"ILi4ELi4ELb0ELb0ELi4ELb0ELb0EE": 0, "ILi4ELi4ELb0ELb0ELi1ELb0ELb0EE": 28}


@pytest.fixture(scope="module")
def step_meta():
    md = kernel_metadata(LIB, ("kernarg_segment_size", "sgpr_spill_count", "private_segment_fixed_size"))
    return {k: v for k, v in md.items() if "step_kernelI" in k}


def test_every_instantiation_is_listed(step_meta):
    assert step_meta, "no step kernels found in liblnw.so"
    for name in step_meta:
        assert any("step_kernel" + frag in name for frag in STEP_KERNELS), f"{name} has no entry in STEP_KERNELS"
    for frag in STEP_KERNELS:
        assert any("step_kernel" + frag in name for name in step_meta), f"step_kernel{frag} not in liblnw.so"


def test_argument_segment(step_meta):
    for name, v in step_meta.items():
        size = v["kernarg_segment_size"]
        assert size < PARENT_KERNARG, f"{name}: {size} B of kernel arguments (the parent had {PARENT_KERNARG})"
        assert size <= REACHED_KERNARG, f"{name}: {size} B of kernel arguments (was {REACHED_KERNARG})"


def test_sgpr_spills(step_meta):
    for name, v in step_meta.items():
        parent, reached, strict = next(x for f, x in STEP_KERNELS.items() if "step_kernel" + f in name)
        n = v["sgpr_spill_count"]
        if strict:
            assert n < parent, f"{name}: {n} spilled SGPRs, not below the parent's {parent}"
        else:
            assert n <= parent, f"{name}: {n} spilled SGPRs, above the parent's {parent}"
        assert n <= reached, f"{name}: {n} spilled SGPRs (was {reached})"


def test_scratch_limits_hold(step_meta):
    for frag, limit in SCRATCH_LIMIT.items():
        for name, v in step_meta.items():
            if "step_kernel" + frag in name:
                assert v["private_segment_fixed_size"] <= limit, \
                    f"{name}: {v['private_segment_fixed_size']} B/lane of scratch (limit {limit})"
