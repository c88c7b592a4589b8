"""Batch event output in CSR form, without a GPU:

  * ivp_event_log_t (include/ivp_hip.h): offsetof / sizeof from gcc equal the ctypes binding, and the #[repr(C)] twin in
    rust/ivp-hip-sys/src/lib.rs lists the same members in the same order;
  * ivp_amd.solve_ivp_batch_events exists, and the header, _lib.EXPORTS and the Rust crate declare the same four functions;
  * the source / destination index arithmetic of the pack kernels (ivp_amd/csrc/event_pack.h, built here for the host
    from the same header) against a numpy pack of a random bounded block: the indices are numpy's, the packed log is
    numpy's bit for bit, and nothing is written outside a run of the packed trajectory range.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ivp_amd
from ivp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ivp_amd", "csrc")
MEMBERS = ["offsets", "t", "y", "capacity", "owned", "device", "passes", "n_events", "total", "staging_bytes"]
FUNCTIONS = {"ivp_batch_solve_events_device", "ivp_batch_solve_events", "ivp_event_log_fetch_device", "ivp_event_log_free"}


def test_event_log_struct_layout_matches_ctypes_and_rust(tmp_path):
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "ivp_hip.h"', 'int main(void) {',
             '  printf("%zu\\n", sizeof(ivp_event_log_t));']
    lines += [f'  printf("{m} %zu %zu\\n", offsetof(ivp_event_log_t, {m}), sizeof(((ivp_event_log_t *)0)->{m}));' for m in MEMBERS]
    lines += ['  return 0;', '}']
    src = tmp_path / "el.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "el"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    assert int(out[0]) == C.sizeof(_lib.EventLogT)
    assert [f[0] for f in _lib.EventLogT._fields_] == MEMBERS
    for line in out[1:]:
        if not line:
            continue
        name, off, size = line.split()
        d = getattr(_lib.EventLogT, name)
        assert (d.offset, d.size) == (int(off), int(size)), name
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivp_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*ivp_event_log_t\s*;", hdr).group(1)
    assert [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()] == MEMBERS
    rust = open(os.path.join(ROOT, "rust", "ivp-hip-sys", "src", "lib.rs")).read()
    rbody = re.search(r"#\[repr\(C\)\]\s*pub struct ivp_event_log_t\s*\{(.*?)\n\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+)\s*:", rbody) == MEMBERS


def test_the_entry_points_are_declared_at_every_boundary():
    assert callable(ivp_amd.solve_ivp_batch_events) and "solve_ivp_batch_events" in ivp_amd.__all__
    hdr = open(os.path.join(ROOT, "include", "ivp_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|void)\s+(ivp_batch_solve_events\w*|ivp_event_log_\w+)\s*\(", hdr, flags=re.M))
    assert declared == FUNCTIONS
    assert FUNCTIONS <= set(_lib.EXPORTS)
    rust = open(os.path.join(ROOT, "rust", "ivp-hip-sys", "src", "lib.rs")).read()
    assert FUNCTIONS <= set(re.findall(r"pub fn (ivp_\w+)\s*\(", rust))
    assert int(re.search(r"#define\s+IVP_HIP_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5   # an additive change


SHIM = r"""
#define IVP_HD inline
#include "event_pack.h"
extern "C" {
unsigned long long ix_src_t(uint32_t i, uint32_t k, size_t j, uint32_t cap, size_t cnt) { return event_src_t(i, k, j, cap, cnt); }
unsigned long long ix_src_y(uint32_t i, uint32_t k, uint32_t c, size_t j, uint32_t cap, uint32_t n, size_t cnt) { return event_src_y(i, k, c, j, cap, n, cnt); }
unsigned long long ix_run(uint32_t i, size_t first, size_t j, size_t B) { return event_run(i, first, j, B); }
unsigned long long ix_hits(uint32_t i, size_t j, size_t cnt) { return event_hits_at(i, j, cnt); }
unsigned long long ix_dst_t(unsigned long long lo, uint32_t k) { return event_dst_t(lo, k); }
unsigned long long ix_dst_y(unsigned long long lo, uint32_t k, uint32_t c, uint32_t n) { return event_dst_y(lo, k, c, n); }
// the pack of a whole range, run by run, in the fallback kernel's decomposition (records strided by k_step)
unsigned pack_range(const double *st_t, const double *st_y, const uint32_t *hits, const unsigned long long *off, double *t, double *y,
                    uint32_t n_events, size_t first, size_t cnt, size_t B, uint32_t cap, uint32_t n, uint32_t k_step)
{
    unsigned bad = 0;
    for (uint32_t i = 0; i < n_events; ++i)
        for (size_t j = 0; j < cnt; ++j)
            for (uint32_t k0 = 0; k0 < k_step; ++k0)
                bad += event_pack_run(st_t, st_y, hits, off, t, y, i, j, first, cnt, B, cap, n, k0, k_step) && k0 == 0;
    return bad;
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("event_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = d / "libshim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    u32, sz, ull = C.c_uint32, C.c_size_t, C.c_ulonglong
    for name, args in (("ix_src_t", [u32, u32, sz, u32, sz]), ("ix_src_y", [u32, u32, u32, sz, u32, u32, sz]), ("ix_run", [u32, sz, sz, sz]),
                       ("ix_hits", [u32, sz, sz]), ("ix_dst_t", [ull, u32]), ("ix_dst_y", [ull, u32, u32, u32])):
        getattr(lib, name).restype = ull
        getattr(lib, name).argtypes = args
    vp = C.c_void_p
    lib.pack_range.restype = C.c_uint
    lib.pack_range.argtypes = [vp, vp, vp, vp, vp, vp, u32, sz, sz, sz, u32, u32, u32]
    return lib


CAP = 5
SENTINEL = np.uint64(0x7FF8DEADBEEF0001)   # a NaN payload no pack produces


def _case(nev, n, cnt, rng, first=3, tail=4):
    """a bounded block of the range [first, first + cnt) of a batch of B, counts from {0, 1, cap - 1, cap} in the range and
    anything up to 2 cap outside it, and the batch-wide offsets"""
    B = first + cnt + tail
    st_t = rng.standard_normal((nev, CAP, cnt))
    st_y = rng.standard_normal((nev, CAP, n, cnt))
    hits = rng.choice(np.array([0, 1, CAP - 1, CAP], dtype=np.uint32), size=(nev, cnt))
    counts = rng.integers(0, 2 * CAP, size=(nev, B)).astype(np.uint32)
    counts[:, first:first + cnt] = hits
    off = np.zeros(nev * B + 1, dtype=np.uint64)
    off[1:] = np.cumsum(counts.reshape(-1).astype(np.uint64))
    return B, st_t, st_y, np.ascontiguousarray(hits), off


def _numpy_pack(nev, n, cnt, first, B, st_t, st_y, hits, off):
    total = int(off[-1])
    t = np.full(total + 3, 0.0).view(np.uint64)
    y = np.full((total + 3, n), 0.0).view(np.uint64)
    t[:] = SENTINEL
    y[:] = SENTINEL
    for i in range(nev):
        for j in range(cnt):
            lo, h = int(off[i * B + first + j]), int(hits[i, j])
            t[lo:lo + h] = st_t[i, :h, j].view(np.uint64)
            y[lo:lo + h] = np.ascontiguousarray(st_y[i, :h, :, j]).view(np.uint64)
    return t, y


@pytest.mark.parametrize("cnt", [1, 63, 65, 130])
@pytest.mark.parametrize("n", [1, 2, 6, 9])
@pytest.mark.parametrize("nev", [1, 3])
def test_pack_indices_reproduce_the_numpy_pack_and_stay_inside_the_runs(shim, nev, n, cnt):
    rng = np.random.default_rng(100000 * nev + 1000 * n + cnt)
    first = 3
    B, st_t, st_y, hits, off = _case(nev, n, cnt, rng, first)
    # ---- the index functions are numpy's own flat indices of the documented shapes ----
    for _ in range(64):
        i, k, c, j = int(rng.integers(nev)), int(rng.integers(CAP)), int(rng.integers(n)), int(rng.integers(cnt))
        assert shim.ix_src_t(i, k, j, CAP, cnt) == np.ravel_multi_index((i, k, j), (nev, CAP, cnt))
        assert shim.ix_src_y(i, k, c, j, CAP, n, cnt) == np.ravel_multi_index((i, k, c, j), (nev, CAP, n, cnt))
        assert shim.ix_hits(i, j, cnt) == np.ravel_multi_index((i, j), (nev, cnt))
        assert shim.ix_run(i, first, j, B) == np.ravel_multi_index((i, first + j), (nev, B))
        lo = int(off[i * B + first + j])
        assert shim.ix_dst_t(lo, k) == lo + k and shim.ix_dst_y(lo, k, c, n) == (lo + k) * n + c
    # ---- the pack ----
    want_t, want_y = _numpy_pack(nev, n, cnt, first, B, st_t, st_y, hits, off)
    for k_step in (1, 3):
        t = np.empty_like(want_t)
        y = np.empty_like(want_y)
        t[:] = SENTINEL
        y[:] = SENTINEL
        bad = shim.pack_range(st_t.ctypes.data, st_y.ctypes.data, hits.ctypes.data, off.ctypes.data, t.ctypes.data, y.ctypes.data,
                              nev, first, cnt, B, CAP, n, k_step)
        assert bad == 0
        assert np.array_equal(t, want_t) and np.array_equal(y, want_y)
        # nothing outside the range's runs: every other record still holds the sentinel
        inside = np.zeros(len(t), dtype=bool)
        for i in range(nev):
            inside[int(off[i * B + first]):int(off[i * B + first + cnt])] = True
        assert (t[~inside] == SENTINEL).all() and (y[~inside] == SENTINEL).all()
        assert (t[inside] != SENTINEL).all()


def test_a_count_that_differs_from_its_run_is_reported_and_clamped(shim):
    """a filling solve that found MORE occurrences than the run has room for (or more than the block holds) writes only
    what fits and is flagged; one that found fewer is flagged too"""
    nev, n, cnt, first = 1, 2, 4, 0
    rng = np.random.default_rng(5)
    st_t = rng.standard_normal((nev, CAP, cnt))
    st_y = rng.standard_normal((nev, CAP, n, cnt))
    room = np.array([2, 2, 2, 2], dtype=np.uint64)
    hits = np.array([[2, 4, 1, CAP + 3]], dtype=np.uint32)        # exact, too many, too few, more than the block holds
    off = np.zeros(cnt + 1, dtype=np.uint64)
    off[1:] = np.cumsum(room)
    t = np.zeros(8 + 2).view(np.uint64)
    y = np.zeros((8 + 2, n)).view(np.uint64)
    t[:] = SENTINEL
    y[:] = SENTINEL
    bad = shim.pack_range(st_t.ctypes.data, st_y.ctypes.data, hits.ctypes.data, off.ctypes.data, t.ctypes.data, y.ctypes.data, nev, first, cnt, cnt, CAP, n, 1)
    assert bad == 3
    wrote = [2, 2, 1, 2]
    for j in range(cnt):
        lo = int(off[j])
        assert np.array_equal(t[lo:lo + wrote[j]], st_t[0, :wrote[j], j].view(np.uint64))
        assert (t[lo + wrote[j]:int(off[j + 1])] == SENTINEL).all()
    assert (t[8:] == SENTINEL).all() and (y[8:] == SENTINEL).all()
