"""Resources of the units kernel compiled for the production configuration
(step_units_prod_kernel, csrc/lnw_kernels.hip ProdCfg), read on the CPU from
the in-tree liblnw.so's gfx950 code object metadata as
tests/test_step_args_cpu.py reads the step kernels'.

The kernel is the generic units kernel's body with the production
configuration's values as constants. What that has to buy is scalar registers:
the generic kernel spills 169 of them (its pin in test_step_args_cpu.py), and
the new one must spill strictly fewer, in the same library, without scratch and
within the 256 VGPRs and the LDS of the generic kernel's launch. The generic
kernel stays in the library: every other configuration runs it.
"""
import pytest

from _codeobj import LIB, kernel_metadata, needs_lib, needs_tools

pytestmark = [needs_lib, needs_tools]

GENERIC = "step_kernelILi4ELi4ELb0ELb0ELi4ELb0ELb0EE"  # step_kernel<4, 4, false, false, 4>
PROD = "step_units_prod_kernel"
KEYS = ("sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size", "vgpr_count", "agpr_count",
        "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size")


@pytest.fixture(scope="module")
def meta():
    md = kernel_metadata(LIB, KEYS)
    gen = [v for k, v in md.items() if GENERIC in k]
    prod = [v for k, v in md.items() if PROD in k]
    assert len(gen) == 1, "the generic units kernel must stay in liblnw.so"
    assert len(prod) == 1, f"{PROD} not in liblnw.so"
    return gen[0], prod[0]


def test_name_is_not_a_step_kernel_instantiation(meta):
    """test_step_args_cpu.py lists every step_kernel<...> instantiation; the new
    kernel has a name of its own and is no entry of that list."""
    md = kernel_metadata(LIB, ("sgpr_spill_count",))
    names = [k for k in md if PROD in k]
    assert names and all("step_kernelI" not in k for k in names)


def test_no_scratch(meta):
    _, prod = meta
    assert prod["private_segment_fixed_size"] == 0
    assert prod.get("vgpr_spill_count", 0) == 0


def test_vgprs(meta):
    _, prod = meta
    assert prod["vgpr_count"] + prod.get("agpr_count", 0) <= 256


def test_fewer_spilled_sgprs_than_the_generic_kernel(meta):
    gen, prod = meta
    print("spilled SGPRs: generic", gen["sgpr_spill_count"], "production", prod["sgpr_spill_count"])
    assert prod["sgpr_spill_count"] < gen["sgpr_spill_count"]


def test_launch_shape_is_the_generic_kernels(meta):
    """The host launches both through rows of the same shape: static LDS no
    larger (the dynamic part is the launch's, computed once for both), the same
    workgroup size and argument segment."""
    gen, prod = meta
    assert prod["group_segment_fixed_size"] <= gen["group_segment_fixed_size"]
    assert prod["max_flat_workgroup_size"] == gen["max_flat_workgroup_size"] == 512
    assert prod["kernarg_segment_size"] == gen["kernarg_segment_size"]
