"""Scratch and spills of the sharded-training kernels (csrc/lnw_ppodist.hip),
read from the in-tree liblnw.so as test_ppo_sample_resources_cpu.py does: a
binary search per list and two copy kernels hold a handful of values, so none
of them has a private segment or spills a register."""
from _codeobj import LIB, kernel_metadata, needs_lib, needs_tools

KERNELS = ("pd_merge_kernel", "pd_pack_obs_kernel", "pd_pack_rows_kernel")
KEYS = ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")


@needs_lib
@needs_tools
def test_ppo_dist_kernels_have_no_scratch_and_no_spills():
    md = kernel_metadata(LIB, KEYS)
    for frag in KERNELS:
        hits = {k: v for k, v in md.items() if frag in k}
        assert len(hits) == 1, f"kernel {frag}: {sorted(hits)} in liblnw.so"
        for name, vals in hits.items():
            for key in KEYS:
                assert vals.get(key) == 0, f"{name}: {key} = {vals.get(key)}"
