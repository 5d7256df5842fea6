"""The kernels of option halo_exact_rows (csrc/elementwise.hip: gather_rows_exact_kernel, scatter_rows_exact_kernel) in the code
objects inside the built library, read as tests/test_bf16_wide_resources.py reads the sweeps' (no GPU needed): they exist and use
no scratch; and what was there before them is what it was -- registers, LDS, scratch and code size of gather_rows_kernel,
scatter_rows_kernel and of one K1s instantiation equal the values recorded from a build of the commit before the option
(metadata only: the notes of the code objects and their symbol tables)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
          "private_segment_fixed_size")

# recorded from a build of the parent commit (1d04136) with the same compiler: FIELDS in order, then the code size in bytes
PARENT = {
    "_ZN4dory18gather_rows_kernelEPfPKfjjPKjj": (17, 0, 32, 0, 0, 0, 0, 916),
    "_ZN4dory19scatter_rows_kernelEPfPKfjjPKjj": (20, 0, 32, 0, 0, 0, 0, 920),
    "_ZN4dory17spmm_sweep_kernelILi32ELi8ELb1ELb0ELb1EEEvNS_8SpmmArgsENS_10BlockedAdjEPKfNS_9SweepArgsE": (104, 0, 106, 0, 0, 102220, 0, 16020),
}


def kernels(lib=None):
    """{mangled kernel name: FIELDS in order + (code size,)} over every gfx950 code object of the library"""
    lib = lib or os.path.join(ROOT, "dorylus_amd", "libdorylus_hip.so")
    assert os.path.exists(lib), "the library is not built"
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("llvm tools missing")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(lib, os.path.join(d, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            run = lambda *a: subprocess.run([os.path.join(LLVM, "llvm-readelf"), *a, f], cwd=d, check=True, capture_output=True, text=True).stdout
            sizes = {m.group(2): int(m.group(1)) for m in re.finditer(r"^\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)$", run("-sW"), re.M)}
            for entry in re.split(r"\n  - (?=\.agpr_count:)", run("--notes")):
                name = re.search(r"^\s+\.name:\s+(\S+)$", entry, re.M)
                if not name or name.group(1) not in sizes:
                    continue
                vals = []
                for fld in FIELDS:
                    m = re.search(r"^\s*(?:- )?\.%s:\s+(\d+)$" % fld, entry, re.M)
                    vals.append(int(m.group(1)) if m else None)
                out[name.group(1)] = tuple(vals) + (sizes[name.group(1)],)
    return out


@pytest.fixture(scope="module")
def ks():
    return kernels()


def test_exact_kernels_exist_without_scratch(ks):
    for stem in ("gather_rows_exact_kernel", "scatter_rows_exact_kernel"):
        found = {n: v for n, v in ks.items() if stem in n}
        assert len(found) == 1, (stem, sorted(found))
        for n, v in found.items():
            rec = dict(zip(FIELDS, v))
            print(stem, rec, "code bytes", v[-1])
            assert rec["private_segment_fixed_size"] == 0 and rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, (n, rec)
            assert rec["group_segment_fixed_size"] == 0 and rec["vgpr_count"] <= 64, (n, rec)


def test_existing_kernels_keep_the_parents_resources(ks):
    for name, want in PARENT.items():
        assert name in ks, name
        print(name, ks[name])
        assert ks[name] == want, (name, dict(zip(FIELDS + ("code_bytes",), ks[name])), "parent:", want)
