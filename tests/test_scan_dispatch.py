"""The host dispatch of csrc/scans.hip decides which instantiation a call reaches; tests/scan_cases.py lists every reachable
one (ROUTES) with shapes that reach it, and tests/test_gpu_scan_routes.py compares each with the independent model.  A moved
threshold, a changed alignment term or a new template argument would leave a row testing some other kernel than it names
without any GPU test failing -- this test fails instead.  CPU only: it reads the source, models the dispatch in Python, and
reads the kernel descriptors' metadata (symbol names, scratch, spills) of the gfx950 code object; no instruction is inspected."""
import os
import re

import numpy as np
import pytest

import scan_cases as SC
from test_rollout_kernel_resources import LLVM, ROOT, _kernel_meta

SRC = os.path.join(ROOT, "reinforcementlearning.jl_amd", "csrc", "scans.hip")
OBJ = os.path.join(ROOT, "reinforcementlearning.jl_amd", "build", "scans.o")

# (exact text, count): every literal ROUTES and the shapes of scan_cases depend on, as often as the dispatch has it today
PINNED = [
    ("const bool streaming = g.n_slices * g.len >= ((int64_t)1 << 22);", 1),                      # the streaming threshold
    ("const bool env_major = g.slice_stride == 1 && g.v_slice_stride == 1 && g.elem_stride == g.n_slices;", 1),
    ("const uintptr_t al = (uintptr_t)adv | (uintptr_t)r | (uintptr_t)v | (uintptr_t)(ret ? ret : adv);", 1),
    ("if (streaming && env_major && g.n_slices % 4 == 0 && (al & 15) == 0 && (!term || ((uintptr_t)term & 3) == 0)) {", 1),
    ("if constexpr (sizeof(T) == 4) {", 1),                                                        # four per lane: Float32 only
    ("hipLaunchKernelGGL((gae_vec4_kernel<true, 8>), g4,", 1),                                     # the chunk of the vec4 route
    ("hipLaunchKernelGGL((gae_vec4_kernel<false, 8>), g4,", 1),
    ("hipLaunchKernelGGL((gae_kernel<T, WR_, 128 / sizeof(T), NT_>), grid,", 1),                   # chunk 32 / 16
    ("if (streaming) LAUNCH_GAE(true, true);", 1),
    ("else LAUNCH_GAE(true, false);", 1),
    ("if (streaming) LAUNCH_GAE(false, true);", 1),
    ("else LAUNCH_GAE(false, false);", 1),
    ("hipLaunchKernelGGL((discount_kernel<T, REDUCED>), dim3((int)((g.n_slices + 255) / 256)), dim3(256), 0,", 1),
    ("if (g.n_slices == 0 || (g.len == 0 && !REDUCED)) return RLHIP_OK;", 1),                      # len = 0 launches only REDUCED
    ("#pragma unroll 4", 1),                                                                       # the discount loop's "chunk"
    ("*g = {1, n1, 1, n1, n1 + 1};", 1),                                                           # scan_geom: dims = 0
    ("*g = {n2, n1, 1, n1, n1 + 1};", 1),                                                          # dims = 1
    ("*g = {n1, n2, n1, 1, 1};", 1),                                                               # dims = 2
    ("return gae_impl<float>(adv, ret, r, v, n_env, T, gamma, lambda, terminal, 2, as_stream(stream));", 1),
    ("return gae_impl<float>(adv, nullptr, r, v, n1, n2, gamma, lambda, terminal, dims, as_stream(stream));", 1),
    ("return gae_impl<double>(adv, nullptr, r, v, n1, n2, gamma, lambda, terminal, dims, as_stream(stream));", 1),
]


def test_scan_dispatch_literals_match_the_route_table():
    src = open(SRC).read()
    moved = [(p, n, src.count(p)) for p, n in PINNED if src.count(p) != n]
    assert not moved, ("a dispatch line of csrc/scans.hip changed -- re-derive ROUTES and the shapes of tests/scan_cases.py so that "
                       f"every instantiation is still reached, then this list: {moved}")
    assert len(re.findall(r"\bgae_impl<(?:float|double)>\(", src)) == 3  # no further caller that could pass `ret`
    assert SC.STREAM_MIN == 1 << 22


def dispatch(entry, n1, n2, dims, misaligned=None, has_term=True):
    """scan_geom / discount_impl / gae_impl restated: the mangled template name a call launches (None: no launch)"""
    n_slices, length = {0: (1, n1), 1: (n2, n1), 2: (n1, n2)}[dims]
    if entry.startswith("rlhip_discount_rewards"):
        reduced = "_reduced_" in entry
        if n_slices == 0 or (length == 0 and not reduced):
            return None
        return f"discount_kernelI{'f' if entry.endswith('f32') else 'd'}Lb{int(reduced)}EE"
    if n_slices == 0 or length == 0:
        return None
    ret = entry == "rlhip_gae_returns_f32"
    f32 = entry.endswith("f32")
    streaming = n_slices * length >= 1 << 22
    if f32 and streaming and dims == 2 and n_slices % 4 == 0:
        off16 = misaligned in ("adv", "r", "v") or (misaligned == "ret" and ret)
        off4 = misaligned == "term" and has_term
        if not off16 and not off4:
            return f"gae_vec4_kernelILb{int(ret)}ELi8EE"
    return f"gae_kernelI{'f' if f32 else 'd'}Lb{int(ret)}ELi{32 if f32 else 16}ELb{int(streaming)}EE"


def test_every_case_of_a_route_reaches_the_instantiation_the_row_names():
    for rt in SC.ROUTES:
        aligned = 0
        for c in rt.cases():
            s = SC.storage(c)
            vec4_shape = c.dtype == np.float32 and c.dims == 2 and c.n % 4 == 0 and c.n * c.T >= SC.STREAM_MIN
            if rt.misaligned and vec4_shape:  # this shape reaches the row only through the alignment fall-back
                for which in rt.misaligned:
                    assert dispatch(rt.entry, s["n1"], s["n2"], c.dims, which, c.has_term) == rt.mangled, (rt.id, c.id, which)
                assert dispatch(rt.entry, s["n1"], s["n2"], c.dims, None, c.has_term) != rt.mangled
                continue
            assert dispatch(rt.entry, s["n1"], s["n2"], c.dims, None, c.has_term) == rt.mangled, (rt.id, c.id)
            aligned += 1
        assert aligned, rt.id
        assert rt.ch == {"discount": 4, "gae_kernelIf": 32, "gae_kernelId": 16, "gae_vec4": 8}[
            next(k for k in ("discount", "gae_kernelIf", "gae_kernelId", "gae_vec4") if rt.mangled.startswith(k))]


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
def test_code_object_holds_exactly_the_listed_instantiations_without_scratch(tmp_path):
    import __graft_entry__ as g

    g.build()
    meta = _kernel_meta(OBJ, str(tmp_path))
    found = {}
    for name, m in meta.items():
        hit = re.search(r"((?:discount_kernel|gae_vec4_kernel|gae_kernel)I(?:f|d|Lb[01]E|Li\d+E)+E)Ev", name)
        if hit:
            assert hit.group(1) not in found, name
            found[hit.group(1)] = m
    listed = {r.mangled for r in SC.ROUTES} | set(SC.UNREACHABLE)
    assert set(found) == listed, (sorted(set(found) - listed), sorted(listed - set(found)))
    assert len(found) == len(meta) == 14, sorted(meta)  # scans.hip holds nothing else
    bad = [f"{k}: {m['vspill']} spilled VGPRs, {m['scratch']} B of scratch" for k, m in found.items() if m["vspill"] or m["scratch"]]
    assert not bad, "\n".join(bad)
