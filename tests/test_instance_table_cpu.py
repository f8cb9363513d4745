"""tests/instance_table.py against the built libraries, without a GPU: the table's rows (plus its exclusion list) are
exactly the kernels the libraries hold, and every row's launcher call selects the instance the row names — asked of
the library's launch record in dry-run, on poisoned host buffers that must come back untouched."""
import collections
import os
import re
import shutil
import subprocess
import sys

import pytest

import gpusolve as gsv
import instance_table as IT

LIBS = {IT.HIP: gsv._abi.KERNEL_LIB, IT.TRANSFER: gsv._abi.TRANSFER_LIB}
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def tool(name):
    """A binary tool: on PATH, or in the ROCm installation's LLVM directory. Missing is a failure."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for path in (shutil.which(name), os.path.join(rocm, "llvm", "bin", name), os.path.join(rocm, "lib", "llvm", "bin", name)):
        if path and os.path.exists(path):
            return path
    pytest.fail(f"{name} not found (PATH, {rocm}/llvm/bin): the inventory needs it")


def normalise(name):
    """tools/isa_digest.py's: without `(anonymous namespace)::` and the argument list; and without the return type."""
    name = name.replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    depth = 0
    for i, c in enumerate(name):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            return name[:i]
    return name


def inventory(lib, tmp):
    """The gfx950 kernels of a built library: its .hip_fatbin section, unbundled, the code object's FUNC symbols."""
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
    subprocess.run([tool("objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}",
                    f"--output={co}"], check=True)
    syms = subprocess.run([tool("llvm-readelf"), "--syms", "--wide", co], capture_output=True, text=True, check=True).stdout
    mangled = [line.split()[-1] for line in syms.splitlines() if len(line.split()) >= 8 and line.split()[3] == "FUNC"]
    names = subprocess.run([tool("c++filt")], input="\n".join(mangled), capture_output=True, text=True,
                           check=True).stdout.splitlines()
    return sorted({normalise(n) for n in names})


@pytest.mark.parametrize("lib,count", [(IT.HIP, 147), (IT.TRANSFER, 17)])
def test_table_is_the_inventory(lib, count, tmp_path):
    """Rows and exclusions are exactly the kernels of the built library, no row name twice, the families' counts the
    documented ones."""
    inv = inventory(LIBS[lib], str(tmp_path))
    assert len(inv) == count, len(inv)
    names = [r.name for r in IT.rows() if r.lib == lib]
    twice = [n for n, c in collections.Counter(names).items() if c > 1]
    assert not twice, twice
    excluded = set(IT.EXCLUDED[lib])
    assert not (excluded & set(names))
    assert set(names) | excluded == set(inv), (sorted(set(inv) - set(names) - excluded),
                                               sorted((set(names) | excluded) - set(inv)))
    for r in IT.rows():
        if r.lib == lib:
            assert r.name in r.launches and set(r.launches) <= set(inv), r


def test_family_counts():
    got = collections.Counter(r.family for r in IT.rows())
    assert dict(got) == IT.FAMILY_COUNTS
    assert sum(c for f, c in IT.FAMILY_COUNTS.items() if not f.endswith("_pa")) == 147
    assert sum(c for f, c in IT.FAMILY_COUNTS.items() if f.endswith("_pa")) == 9
    assert sorted(IT.EXCLUDED[IT.TRANSFER]) == sorted(["k_rhs", "k_bfac", "k_copy", "k_fill", "k_axpy", "k_interpolate",
                                                       "k_restrict", "k_sumsq_finish"])
    assert all(IT.EXCLUDED[IT.TRANSFER].values()) and IT.EXCLUDED[IT.HIP] == {}
    knobbed = sorted(r.name for r in IT.rows() if r.env)
    assert knobbed == sorted(["k_rr2<0, 2, true>", "k_rr2<0, 2, false>", "k_tb3y<true, true, true, false>",
                              "k_tb3y<true, false, true, false>", "k_fmg_prolong<true>", "k_fmg_prolong_pa<true>"])
    for r in IT.rows():  # no row needs more than a few million points
        n = 1
        for d in r.shape:
            n *= d
        assert n <= 4_000_000, r


@pytest.mark.parametrize("row", [r for r in IT.rows() if not r.env], ids=lambda r: r.id)
def test_selection(row):
    """The row's launcher call, in dry-run on poisoned host buffers: return code 0, the launch record holds the
    row's kernel (after k_pro_strip<false> for a column-block prolongation pair), no buffer touched."""
    IT.dry_run(row, True)
    try:
        R = IT.HostSide()
        rc, names = IT.launch(row, R)
    finally:
        assert IT.dry_run(row, False) == 1
    assert rc == 0, (row, rc)
    assert names == row.launches, (row, names)
    assert R.untouched(), f"{row}: the dry run read into or wrote a buffer"
    assert IT.take_record(row) == []


def test_selection_under_switches():
    """The six instances that only A/B switches select below 2^25 points: their rows in one child process."""
    rows = [r for r in IT.rows() if r.env]
    env = dict(os.environ, **IT.KNOBS)
    assert all(r.env == IT.KNOBS for r in rows)
    probe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "instance_probe.py")
    r = subprocess.run([sys.executable, probe, "dry"], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["ok " + x.name for x in rows]


def test_dry_run_is_per_thread_and_off_by_default():
    """The flag starts off, gs_launch_dry_run returns the previous setting, and another thread's flag is its own."""
    import threading
    k = gsv.kernels()
    assert k.gs_launch_dry_run(1) == 0 and k.gs_launch_dry_run(1) == 1
    seen = []
    t = threading.Thread(target=lambda: seen.append(k.gs_launch_dry_run(0)))
    t.start()
    t.join()
    assert seen == [0]
    assert k.gs_launch_dry_run(0) == 1 and k.gs_launch_dry_run(0) == 0
    assert k.gs_launch_record(None, 0) == -1


def test_dry_run_skips_the_runtime_calls_that_stand_in_for_a_kernel():
    """gs_copy's memcpy for operands without a common 16-byte phase, and the memset of the one partial of an empty
    level in gs_jacobi_sweep_norm / gs_residual: return code 0, nothing recorded, no buffer touched."""
    import ctypes as C
    k = gsv.kernels()
    S = C.byref(IT.stencil_abi("unit"))
    row = IT.Row("one-off", "k_copy", "copy", (64,))
    IT.dry_run(row, True)
    try:
        IT.take_record(row)
        a, b, p = IT.HostBuf(80, 8, IT.POISON_OUT), IT.HostBuf(80, 9, IT.POISON_IN), IT.HostBuf(16, 8, IT.POISON_OUT)
        assert (a.ptr ^ b.ptr) & 15
        assert k.gs_copy(a.ptr, b.ptr, 64, None) == 0
        empty = gsv.gs_level(0, 5, 5, 16, 16 * 7, 0, 0.1)
        assert k.gs_jacobi_sweep_norm(S, C.byref(empty), 0, 0.8, 1.0, b.ptr, a.ptr, b.ptr, None, p.ptr, None) == 0
        assert k.gs_residual(S, C.byref(empty), 0, 1.0, b.ptr, b.ptr, None, a.ptr, p.ptr, None) == 0
        assert IT.take_record(row) == []
        assert a.untouched() and b.untouched() and p.untouched()
    finally:
        IT.dry_run(row, False)
