"""The gfx950 code objects' kernel metadata, read on the CPU from the in-tree
liblnw.so (llvm-objcopy, the offload bundler, llvm-readelf --notes).

TEST INFRASTRUCTURE: shared by the *_resources_cpu.py tests, test_step_args_cpu.py
and test_units_prod_cpu.py, which keep their own tables of limits.
"""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "littoral-naval-warfare-marl_amd", "lnw", "liblnw.so")
LLVM = "/opt/rocm/lib/llvm/bin"


def tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="liblnw.so not built")
needs_tools = pytest.mark.skipif(not (tool("llvm-objcopy") and tool("clang-offload-bundler") and tool("llvm-readelf")),
                                 reason="ROCm LLVM tools not found")


@functools.lru_cache(maxsize=None)
def _extract(lib, mtime, size):
    """llvm-readelf's notes of every gfx950 code object in the library, one text per offload bundle."""
    texts = []
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", lib,
                        os.path.join(tmp, "host.so")], check=True, capture_output=True)
        data = open(fat, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts = [m.start() for m in re.finditer(re.escape(magic), data)]
        for n, a in enumerate(starts):
            b = starts[n + 1] if n + 1 < len(starts) else len(data)
            part, co = os.path.join(tmp, f"b{n}.bin"), os.path.join(tmp, f"co{n}.o")
            with open(part, "wb") as f:
                f.write(data[a:b])
            subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"],
                           check=True, capture_output=True)
            texts.append(subprocess.run([tool("llvm-readelf"), "--notes", co], check=True, capture_output=True,
                                        text=True).stdout)
    return texts


def kernel_metadata(lib, keys):
    """{kernel name: {key: int}} over every code object in the library's
    .hip_fatbin (one offload bundle per translation unit). The library is taken
    apart once per process and state of the file."""
    out = {}
    st = os.stat(lib)
    for notes in _extract(os.path.abspath(lib), st.st_mtime_ns, st.st_size):
        # one "- .agpr_count: ..." list item per kernel under amdhsa.kernels
        for item in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            m = re.search(r"\.name:\s+(\S+)", item)
            if not m:
                continue
            vals = {}
            for k in keys:
                v = re.search(r"\.%s:\s+(\d+)" % re.escape(k), item)
                if v:
                    vals[k] = int(v.group(1))
            out[m.group(1)] = vals
    return out


def kernel_scratch(lib):
    """{kernel name: private segment bytes per lane}."""
    key = "private_segment_fixed_size"
    return {name: v[key] for name, v in kernel_metadata(lib, (key,)).items() if key in v}
