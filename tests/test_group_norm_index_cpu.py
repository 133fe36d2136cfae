"""csrc/gn_index.h - the index arithmetic that replaced the integer divisions of the GroupNorm kernels (a thread's pixel slot, an LDS
item's slot, the group of each channel of a 16-byte chunk) - compiled as HOST code and compared with `/`: tests/gn_index_check.cpp walks
gn_div over every divisor up to 8192 and every dividend below 2^14 (the kernels stay below both), and gn_chunk_groups over every chunk of
every C <= 2560 for every group count 1 .. 32 dividing C (SD's 32 and 1, 2, 4, 8, 16 among them).  norm.hip includes the same header."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_norm_index_arithmetic_equals_integer_division(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "gn_index_check")
    c = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "gn_index_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "bad 0" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_kernels_use_the_checked_header():
    src = open(os.path.join(ROOT, "edgestyle_amd", "csrc", "norm.hip")).read()
    assert '#include "gn_index.h"' in src and "gn_chunk_groups(" in src and "gn_div(" in src
    body = src[src.index("void gn_slab_kernel("):src.index("int gn_slab_gpb(")]
    assert "/ cpg;" not in body.replace("C / p.groups", "") and ") / cpg" not in body, "an integer division by cpg is back in gn_slab_kernel"
