"""tools/kernel_fingerprint.py on a two-kernel toy source: the fingerprint of a kernel is
its machine code and descriptor, so it ignores comments and whitespace and changes, for
that kernel alone, when the kernel's code changes.  Needs hipcc (cross-compiles for gfx950
without a GPU)."""
import importlib.util
import os
import shutil
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"))
              if c and os.path.exists(c)), None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not found")

TOY = """#include <hip/hip_runtime.h>
__global__ void scale_kernel(float* p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = p[i] * 3.0f;
}
template <int K>
__global__ void shift_kernel(int* p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = p[i] + K;
}
template __global__ void shift_kernel<7>(int*, int);
"""
SCALE = "scale_kernel(float*, int)"
SHIFT = "void shift_kernel<7>(int*, int)"


def _tool():
    spec = importlib.util.spec_from_file_location(
        "kernel_fingerprint", os.path.join(ROOT, "tools", "kernel_fingerprint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def prints(tmp_path_factory):
    """Fingerprints of the toy source, of a comment / whitespace edit of it, and of an edit
    of one constant in scale_kernel (compiled once, at the same time)."""
    kf = _tool()
    tmp = tmp_path_factory.mktemp("fingerprint")
    variants = {
        "base": TOY,
        "cosmetic": "// a comment\n\n" + TOY.replace("  const int i =", "\n    const  int  i  =  ")
                    .replace("if (i < n) p[i] = p[i] * 3.0f;", "if (i < n)  // scale\n    p[i] = p[i] * 3.0f;"),
        "constant": TOY.replace("3.0f", "5.0f"),
    }
    assert variants["cosmetic"] != TOY and variants["constant"] != TOY

    def one(item):
        name, text = item
        src = tmp / f"{name}.hip"
        src.write_text(text)
        obj = kf.compile_device(HIPCC, kf.device_flags(), str(src), str(tmp / f"{name}.o"))
        return name, kf.fingerprint_object(obj)

    with ThreadPoolExecutor(max_workers=3) as ex:
        return kf, tmp, dict(ex.map(one, variants.items()))


def test_both_kernels_are_found(prints):
    _, _, fp = prints
    assert sorted(fp["base"]) == sorted([SCALE, SHIFT])
    for k in (SCALE, SHIFT):
        assert len(fp["base"][k]["code"]) == 64 and len(fp["base"][k]["kd"]) == 64
        assert fp["base"][k]["bytes"] > 0
    assert fp["base"][SCALE]["code"] != fp["base"][SHIFT]["code"]


def test_comment_and_whitespace_leave_fingerprints_equal(prints):
    _, _, fp = prints
    assert fp["cosmetic"] == fp["base"]


def test_constant_changes_that_kernel_only(prints):
    _, _, fp = prints
    assert fp["constant"][SCALE]["code"] != fp["base"][SCALE]["code"]
    assert fp["constant"][SHIFT] == fp["base"][SHIFT]


def test_diff_lists_only_old_only_new_and_changed(prints, capsys):
    kf, _, fp = prints
    old = {"toy.hip": dict(fp["base"], **{"void gone_kernel<3, false>(int*)": fp["base"][SHIFT]})}
    new = {"toy.hip": dict(fp["constant"], **{"void kept_kernel<3>(int*)": fp["base"][SHIFT]})}
    assert kf.diff(old, new, []) == 1
    out = capsys.readouterr().out
    assert "only in OLD: 1" in out and "only in NEW: 1" in out and "changed: 1" in out
    assert f"toy.hip: {SCALE}  [code]" in out
    # a rename maps the parameter that went away; an unchanged pair reports nothing
    assert kf.diff(old, new, [r"gone_kernel<3, false>=>kept_kernel<3>"]) == 1
    out = capsys.readouterr().out
    assert "only in OLD: 0" in out and "only in NEW: 0" in out and "changed: 1" in out
    assert kf.diff({"toy.hip": fp["base"]}, {"toy.hip": fp["cosmetic"]}, []) == 0
