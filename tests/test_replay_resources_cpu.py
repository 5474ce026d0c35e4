"""Resources of the DDQN replay kernels (csrc/lnw_replay.hip), read from the
in-tree liblnw.so as test_ppo_dist_resources_cpu.py does: a per-env sum and a
copy kernel hold a handful of values, so neither has a private segment, spills a
register or uses LDS, and their register counts are the ones DESIGN.md "DDQN
replay" records."""
from _codeobj import LIB, kernel_metadata, needs_lib, needs_tools

ZERO = ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size")
# kernel: (VGPRs, SGPRs) of the gfx950 build
KERNELS = {"rp_mark_kernel": (10, 20), "rp_pack_kernel": (24, 73)}


@needs_lib
@needs_tools
def test_replay_kernels_resources():
    md = kernel_metadata(LIB, ZERO + ("vgpr_count", "sgpr_count"))
    for frag, (vgpr, sgpr) in KERNELS.items():
        hits = {k: v for k, v in md.items() if frag in k}
        assert len(hits) == 1, f"kernel {frag}: {sorted(hits)} in liblnw.so"
        for name, vals in hits.items():
            for key in ZERO:
                assert vals.get(key) == 0, f"{name}: {key} = {vals.get(key)}"
            assert (vals.get("vgpr_count"), vals.get("sgpr_count")) == (vgpr, sgpr), (name, vals)
