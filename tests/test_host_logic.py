"""CPU-side tests (no GPU): packer validation, generated header, C-ABI library loading / symbol
export / argument errors, and the 'no CPU fallback' contract of the Python API."""
import ctypes
import os
import shutil

import numpy as np
import pytest

from conftest import ROOT, make_robot

from rbdreference_amd import pack_robot, iiwa_like, quadruped_like, atlas_like, random_tree
from rbdreference_amd.packer import emit_header
from rbdreference_amd.robot import Link, Robot

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


def test_pack_builtin_topologies():
    m7, m12, m30 = pack_robot(iiwa_like()), pack_robot(quadruped_like()), pack_robot(atlas_like())
    assert m7.parent == [-1, 0, 1, 2, 3, 4, 5] and m7.max_depth == 7
    assert m12.parent == [-1, 0, 1, -1, 3, 4, -1, 6, 7, -1, 9, 10] and m12.max_depth == 3
    assert m30.n == 30 and m30.max_depth == 10
    assert m30.ancestors(10) == [0, 1, 2, 4, 5, 6, 7, 8, 9]
    # iiwa joint frames are related by multiples of pi/2: X_tree entries are exactly 0 / +-1 / offsets
    E = m7.Xtree[:, :3, :3]
    assert set(np.unique(E)) <= {-1.0, 0.0, 1.0}
    for m in (m7, m12, m30):
        for i in range(m.n):
            w = np.linalg.eigvalsh(m.I[i])
            assert w.min() > 0, f"{m.name} body {i}: spatial inertia not positive definite"


def test_hash_is_stable_and_sensitive():
    a, b = pack_robot(iiwa_like()), pack_robot(iiwa_like())
    assert a.hash == b.hash and len(a.hash) == 16
    r = iiwa_like()
    r._I[3] = r._I[3] * 1.0000001
    assert pack_robot(r).hash != a.hash


def test_packer_rejects_unsupported_robots():
    r = iiwa_like(); r.floating_base = True              # claims a floating base without its layout (num_vel, S, indices)
    with pytest.raises(ValueError):
        pack_robot(r)
    r = iiwa_like(); r._S[2] = np.array([0.6, 0.8, 0, 0, 0, 0.0])
    with pytest.raises(ValueError, match="coordinate axis"):
        pack_robot(r)
    r = iiwa_like(); f0 = r._Xfunc[1]; r._Xfunc[1] = lambda q: f0(2 * q)      # not X_J(q) X(0)
    with pytest.raises(ValueError, match="unsupported joint convention"):
        pack_robot(r)
    r = iiwa_like(); r._I[0][0, 1] += 0.01                                     # asymmetric inertia
    with pytest.raises(ValueError, match="symmetric"):
        pack_robot(r)
    with pytest.raises(ValueError):
        Robot("bad", [Link("a", 0, 2, (0, 0, 0))])                             # parent must precede


def test_header_is_bit_exact():
    m = pack_robot(random_tree([-1, 0, 0, 2], seed=3))
    h = emit_header(m)
    assert f"constexpr int N = {m.n};" in h and f"0x{m.hash}ULL" in h
    # hex-float literals round-trip exactly
    row = h.split("constexpr double IM[N][36] = {")[1].split("};")[0].strip().splitlines()[0]
    vals = [float.fromhex(t) if "x" in t else float(t) for t in row.strip(" {},").split(", ")]
    assert np.array_equal(np.array(vals), m.I[0].reshape(-1))


def _prebuilt(name):
    from rbdreference_amd.build import lib_path
    return lib_path(pack_robot(make_robot(name)))


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_capi_library_builds_loads_and_exports_every_symbol():
    """Cross-compiles the small prismatic test robot if its library is stale (about a minute)."""
    from rbdreference_amd._lib import EXPORTED_SYMBOLS, RbdLibrary, RbdModelInfo
    robot = make_robot("random_prismatic_n6")
    m = pack_robot(robot)
    lib = RbdLibrary(m, build=True)
    # every function include/rbd_hip.h declares is exported
    hdr = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    import re
    declared = set(re.findall(r"\b(rbd_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(EXPORTED_SYMBOLS)
    for s in declared:
        assert hasattr(lib.lib, s), s
    info = RbdModelInfo()
    assert lib.lib.rbd_model_info(ctypes.byref(info)) == 0
    assert info.n == 6 and list(info.parent[:6]) == m.parent and f"{info.hash:016x}" == m.hash
    assert list(info.joint_type[:6]) == m.jtype and list(info.joint_axis[:6]) == m.axis
    assert info.name.decode() == "random_prismatic_n6"
    # argument errors are reported before anything touches a GPU
    L = lib.lib
    assert L.rbd_rnea_f32(None, None, None, -9.81, 4, None, None, None, None, None) == -1
    assert b"non-null" in L.rbd_last_error()
    assert L.rbd_rnea_grad_f64(1, 1, None, -9.81, 0, -5, None, 1, None) == -1
    wsb = L.rbd_minv_workspace_bytes(10, 4)
    assert wsb in (0, 10 * 6 * 12 * 4)          # 0: fused one-lane minv kernel (no workspace)
    if wsb:
        assert L.rbd_minv_f32(1, 4, 1, 1, None, 0, None) == -3
    assert L.rbd_minv_f32(1, 4, 1, None, None, 0, None) == -1
    assert L.rbd_minv_workspace_bytes(10, 2) == 0
    assert L.rbd_rnea_f32(None, None, None, -9.81, 0, None, None, None, None, None) == 0   # B = 0: no-op
    from rbdreference_amd.packer import ABI_VERSION
    assert L.rbd_abi_version() == ABI_VERSION == 2


def test_every_prebuilt_library_matches_its_robot():
    """Libraries present in-tree (they travel to the GPU box) must be the ones for today's robots."""
    from rbdreference_amd._lib import RbdLibrary
    found = 0
    for name in ("iiwa_like", "quadruped_like", "atlas_like", "random_tree_n9", "random_prismatic_n6"):
        if os.path.exists(_prebuilt(name)):
            RbdLibrary(pack_robot(make_robot(name)), build=False)     # raises on any mismatch
            found += 1
    if HAVE_HIPCC:
        assert found >= 1


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    import rbdreference_amd.build as b
    from rbdreference_amd._lib import RbdLibrary
    monkeypatch.setattr(b, "BUILD_DIR", str(tmp_path))
    with pytest.raises(FileNotFoundError, match="no CPU fallback"):
        RbdLibrary(pack_robot(random_tree([-1, 0], seed=99)), build=False)


def test_api_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu tests")
    if not os.path.exists(_prebuilt("iiwa_like")):
        pytest.skip("iiwa library not built")
    from rbdreference_amd import RBDReference
    rbd = RBDReference(iiwa_like(), build=False)
    q = np.zeros(7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rbd.rnea(q, q, q)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rbd.minv(torch.zeros(3, 7))


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "rbdreference_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f
                assert "/root/reference" not in txt or f.endswith((".py", ".hip", ".h")), f


@pytest.mark.skipif(not HAVE_HIPCC, reason="needs the ROCm LLVM tools")
def test_kernels_of_built_libraries_do_not_spill():
    """every kernel of every test robot, fp32 AND fp64 (the reference's own arithmetic), is free of
    scratch memory (spills are HBM traffic, §3) -- without exception since the fp64 gradient of the 30-body robot runs
    the workspace tree kernel (rbd_idsva_tree_ws.h) instead of the two-lane column kernel, which is no longer built
    for it.  Checked on whatever per-robot libraries are present (build() makes all of them); reads the code-object
    metadata only, no GPU."""
    import glob
    import subprocess
    import sys
    libs = sorted(glob.glob(os.path.join(ROOT, "rbdreference_amd", "_build", "librbd_*_*.so")))
    libs = [l for l in libs if l.count(".") == 1]            # skip tagged experiment builds and family libraries
    if not libs:
        pytest.skip("no per-robot library built yet")
    bad = []
    for lib in libs:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), lib],
                             capture_output=True, text=True, check=True).stdout
        robot = os.path.basename(lib)[len("librbd_"):].rsplit("_", 1)[0]
        for line in out.splitlines():
            name = line.split("vgpr=")[0].strip()
            spill = int(line.rsplit("spill=", 1)[1])
            scratch = int(line.split("scratch=")[1].split()[0])
            # `spill` with scratch == 0 are copies into the accumulator half of a lone wave's 512-entry
            # register file (v_accvgpr_write / read): registers, not memory traffic
            if scratch:
                bad.append((os.path.basename(lib), name, spill, scratch))
            if robot == "atlas_like":
                assert not name.startswith("rnea_grad_kernel<double"), "the spilling two-lane fp64 kernel is back in the Atlas library"
    assert not bad, bad


def test_no_vector_write_sits_in_an_exec_masked_window_and_no_kernel_calls_out():
    """The round-3 aperture fault (docs/NOTEBOOK.md 3.1 a' (xv)) was a register copy the compiler had placed at the head of
    the ELSE block of the device library's lane-masked `if (|x| large)`, before EXEC is restored there.  Round 4 removed
    the library sin / cos (csrc/rbd_sincos.h is straight-line code); this guards the ISA of whatever libraries are built:
    no vector instruction between a label `s_cbranch_execz` jumps to and the first rewrite of EXEC, no out-of-line
    call, and no lane-masked if / ELSE at all in the fp64 kernels that keep state in AGPRs (tools/isa_exec_audit.py;
    reads the code objects, no GPU)."""
    import glob
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_exec_audit
    libs = sorted(glob.glob(os.path.join(ROOT, "rbdreference_amd", "_build", "librbd_*_*.so")))
    libs = [l for l in libs if l.count(".") == 1 and any(k in l for k in ("iiwa_like", "random_chain_n7", "atlas_like", "random_twochains_n18", "fb_quadruped_like"))]
    if not libs:
        pytest.skip("no per-robot library built yet")
    for lib in libs:
        for dem, n, else_blocks, execz_targets, calls, masked in isa_exec_audit.audit(lib):
            assert not masked, (os.path.basename(lib), dem, masked[:4])
            assert calls == 0, (os.path.basename(lib), dem, "out-of-line call")
            if "double" in dem and ("rnea_grad_idsva_kernel" in dem or "rnea_grad_kernel<" in dem):
                assert else_blocks == 0, (os.path.basename(lib), dem, else_blocks)


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_capi_host_code_is_clean_under_asan_and_ubsan():
    """SURVEY.md section 5 / VERDICT r3 item 9: the host side of the C-ABI (argument, alignment and workspace checks,
    option atomics, kernel-name queries, the workspace pool) compiled with -fsanitize=address,undefined (host only) and
    driven without a GPU by tools/asan_host_checks.py in a child process that preloads the sanitizer runtime.  A report
    aborts the child.  Small robots: a 4-body tree (one-lane kernels) -- the launch logic is the same templates for every
    robot.  On a machine with a GPU the child's first HIP call initialises the device under ASan, which aborts in the HIP
    runtime (out of memory) before any check runs: the sanitizer checks are for GPU-less machines only."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("host sanitizer checks run on a machine without a GPU (ASan aborts in the HIP runtime's device set-up)")
    from rbdreference_amd.build import build_sanitized, sanitizer_runtime
    from rbdreference_amd.robot import random_tree
    m = pack_robot(random_tree([-1, 0, 0, 2], seed=3, name="asan_probe_n4"))
    lib = build_sanitized(m)
    assert lib.endswith(".asan.so") and os.path.exists(lib)
    preload = ":".join(p for p in (sanitizer_runtime(), os.environ.get("LD_PRELOAD", "")) if p)   # the ASan runtime first
    env = dict(os.environ, LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asan_host_checks.py"), lib], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "asan host checks OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_robot_name_cannot_inject_code_into_the_generated_header():
    """the name comes from the caller or from a URDF's <robot name=...>; the generated header is
    compiled and dlopen'ed in-process, so only [A-Za-z0-9_] (at most 63 characters) may reach it or the file name."""
    from rbdreference_amd.build import lib_path
    from rbdreference_amd.packer import emit_header, safe_name
    evil = 'x"; static int pwn = system("id"); //\\ \n#error boom \u00e9'
    m = pack_robot(iiwa_like(), evil)
    hdr = emit_header(m)
    line = [l for l in hdr.splitlines() if l.startswith("#define RBD_MODEL_NAME")][0]
    inside = line.split('"')[1]
    assert line.count('"') == 2 and inside == safe_name(evil) and inside.replace("_", "").isalnum() and inside.isascii()
    assert "system(" not in hdr and "#error" not in hdr and "\\" not in hdr
    assert all(ch.isalnum() or ch in "_." for ch in os.path.basename(lib_path(m)))
    assert len(safe_name("a" * 200)) == 63 and safe_name("") == "robot"
    assert pack_robot(iiwa_like(), evil).hash == pack_robot(iiwa_like()).hash      # the name is not part of the model


def _fresh_robot(name, parents, seed):
    """A robot whose libraries do not exist yet: whatever an earlier run left behind is removed first."""
    import glob
    from rbdreference_amd.build import lib_path
    from rbdreference_amd.packer import pack_robot
    from rbdreference_amd.robot import random_tree
    m = pack_robot(random_tree(parents, seed=seed, name=name))
    for f in glob.glob(lib_path(m)[:-3] + "*"):
        os.remove(f)
    return m


def test_first_use_family_library_builds_within_its_bound_and_says_what_it_lacks():
    """a robot that has never been built answers its first call from a FAMILY library (COMMON + one
    family of entry points + stubs) instead of waiting for the whole library.  No GPU here: the bound is on the build
    (hipcc cross-compiles), the library must load, carry the robot, export every symbol of the header, and a stub
    must say RBD_ERR_NOT_BUILT.  Measured on the 8-core build container: rnea 4-9 s, gradient 10-16 s for 7 bodies
    (the whole library: 40 s); the bounds below leave room for a loaded machine."""
    import ctypes
    import time
    from rbdreference_amd._lib import EXPORTED_SYMBOLS, RbdModelInfo, _declare
    from rbdreference_amd.build import build_family, family_lib_path, full_library_ready
    m = _fresh_robot("first_use_probe_chain7", [-1, 0, 1, 2, 3, 4, 5], 4242)
    assert not full_library_ready(m)
    t0 = time.time()
    p = build_family(m, "rnea", "f32")
    t_rnea = time.time() - t0
    t0 = time.time()
    pg = build_family(m, "grad", "f32")
    t_grad = time.time() - t0
    assert p == family_lib_path(m, "rnea", "f32") and os.path.exists(p) and os.path.exists(pg)
    assert t_rnea <= 40.0 and t_grad <= 45.0, (t_rnea, t_grad)
    lib = ctypes.CDLL(pg)
    _declare(lib)
    for sym in EXPORTED_SYMBOLS:
        assert hasattr(lib, sym), sym
    info = RbdModelInfo()
    assert lib.rbd_model_info(ctypes.byref(info)) == 0 and f"{info.hash:016x}" == m.hash and info.n == 7
    rc = lib.rbd_minv_f32(None, 4, 1, None, None, 0, None)              # another family's entry point: a stub
    assert rc == -4 and b"not part of this family library" in lib.rbd_last_error()
    buf = ctypes.create_string_buffer(128)
    assert lib.rbd_kernel_name(1, 4, 1 << 20, buf, len(buf)) == 0 and buf.value.startswith(b"rnea_grad_")
    t0 = time.time()
    assert build_family(m, "grad", "f32") == pg and time.time() - t0 < 2.0    # up to date: no compiler run


def test_lazy_library_serves_families_first_and_the_full_library_when_it_is_ready():
    """RbdLibrary on a never-built robot returns at once, hands out entry points from family libraries while the full
    library builds in the background, and `.lib` (the full library) waits for that build."""
    import time
    from rbdreference_amd._lib import RBD_OPT_GRAD_KERNEL, RbdLibrary
    from rbdreference_amd.build import full_library_ready
    m = _fresh_robot("first_use_probe_n2", [-1, 0], 4243)
    t0 = time.time()
    L = RbdLibrary(m, build=True, lazy=True, generic="never")
    assert time.time() - t0 < 2.0 and L._full is None and L._bg is not None
    f = L.fn("rbd_rnea", "f32")
    assert f is not None and (("rnea", "f32") in L._fams or L._full is not None)
    L.set_option(RBD_OPT_GRAD_KERNEL, 3)                                  # remembered, and applied to libraries loaded later
    full = L.lib                                                          # blocks until the background build is done
    assert full_library_ready(m) and full.rbd_get_option(RBD_OPT_GRAD_KERNEL) == 3
    assert L.fn("rbd_rnea", "f32") is not None and L._tls.lib is full
    assert L.info.n == 2


def test_generic_library_loads_exports_its_header_and_serves_a_never_built_robot_at_once():
    """VERDICT r2 'missing 3' (a robot without hipcc and without minutes of compile): the model-handle library of
    include/rbd_generic.h is built ONCE, exports every symbol the header declares, refuses bad descriptions on the
    host (no GPU here), and RbdLibrary hands its entry points out for a never-built robot while the robot's own
    library builds in the background; entry points it does not have still come from a family library."""
    import ctypes
    import re
    import time
    from rbdreference_amd._lib import RbdLibrary
    from rbdreference_amd.build import build_generic, generic_library_ready
    from rbdreference_amd.generic import (GENERIC_EXPORTED_SYMBOLS, GenericModel, RbdModelDesc, load_generic_library,
                                          model_desc_arrays)
    path = build_generic()
    assert generic_library_ready() and os.path.exists(path)
    lib = load_generic_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rbd_generic.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rbd_(?:g_|model_)[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(GENERIC_EXPORTED_SYMBOLS), declared ^ set(GENERIC_EXPORTED_SYMBOLS)
    for sym in GENERIC_EXPORTED_SYMBOLS:
        assert hasattr(lib, sym), sym
    # host-side validation of a description (nothing touches a GPU before the checks pass)
    out = ctypes.c_void_p()
    assert lib.rbd_model_create(None, 0, ctypes.byref(out)) == -1
    m = _fresh_robot("generic_probe_n3", [-1, 0, 0], 4244)
    a = model_desc_arrays(m)
    assert a["X0"].shape == (3, 6, 6) and a["S"][0].sum() == 1.0
    from rbdreference_amd.packer import _joint_X
    for i in range(3):                                   # the three matrices reproduce the joint transform exactly
        for q in (0.3, -1.7):
            want = _joint_X(m.jtype[i], m.axis[i], q) @ m.Xtree[i]
            f1, f2 = (np.sin(q), np.cos(q)) if m.jtype[i] == 0 else (q, 0.0)
            np.testing.assert_allclose(a["X0"][i] + a["Xs"][i] * f1 + a["Xc"][i] * f2, want, rtol=0, atol=1e-15)
    bad = a["parent"].copy(); bad[1] = 2
    d = RbdModelDesc(1, 3, bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), a["joint_type"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                     *[a[k].ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for k in ("S", "X0", "Xs", "Xc", "I", "damping")])
    assert lib.rbd_model_create(ctypes.byref(d), 0, ctypes.byref(out)) == -1 and b"parent[1]" in lib.rbd_g_last_error()
    d.abi_version = 99
    assert lib.rbd_model_create(ctypes.byref(d), 0, ctypes.byref(out)) == -1 and b"abi_version" in lib.rbd_g_last_error()
    # the lazy library: generic first for what it serves, a family library for the rest, the full one when it is ready
    t0 = time.time()
    L = RbdLibrary(m, build=True, lazy=True, generic="auto")
    assert time.time() - t0 < 2.0 and L._full is None
    f = L.fn("rbd_rnea_grad", "f32")
    assert f is not None and (L.served_by_generic() or L._full is not None)
    assert L.kernel_name(1, 4, 1 << 20).startswith(("g_rnea_grad_kernel<float, 8>", "rnea_grad_"))
    assert isinstance(L._generic, GenericModel) and not L._fams
    L.fn("rbd_crba", "f32")                               # round 4: the per-pass surface and crba are served too (fixed base)
    assert L.served_by_generic() or L._full is not None
    for base in ("rbd_rnea_fpass", "rbd_rnea_bpass", "rbd_rnea_grad_fpass_dq", "rbd_rnea_grad_fpass_dqd", "rbd_rnea_grad_bpass_dq",
                 "rbd_rnea_grad_bpass_dqd", "rbd_minv_bpass", "rbd_minv_fpass"):
        assert L._generic.serves(base) and callable(getattr(L._generic, base + "_f64"))
    L.wait_specialized()
    L.fn("rbd_rnea_grad", "f32")
    assert not L.served_by_generic()
    only = RbdLibrary(m, build=True, generic="only")
    only.fn("rbd_minv", "f64")
    assert only.served_by_generic() and only.get_option(0) == 0
    only.fn("rbd_aba", "f32")                              # Minv (tau - c) through rbd_g_forward_dynamics
    assert only.served_by_generic()
    only.fn("rbd_crba", "f32")
    assert only.served_by_generic()
    # a FLOATING-base robot: the model-handle library serves its five products, not the per-pass surface / crba
    from rbdreference_amd.robot import FloatingBaseRobot, random_tree
    fbm = pack_robot(FloatingBaseRobot(random_tree([-1, 0, 1, 0, 3, 3], seed=5, name="t6"), "generic_probe_fb6"))
    gfb = GenericModel(fbm, build=True)
    assert gfb.serves("rbd_rnea_grad") and not gfb.serves("rbd_crba") and not gfb.serves("rbd_minv_bpass")


def test_a_machine_without_hipcc_keeps_serving_from_the_model_handle_library(monkeypatch):
    """No compiler (RBD_HIPCC points nowhere) and a robot that was never built: the background build fails, the
    model-handle library (prebuilt, needs no compiler) keeps answering what it serves, `wait_specialized` returns
    instead of raising (ShardedRBD can run), and an entry point it does not have reports the build error."""
    from rbdreference_amd._lib import RbdLibrary
    from rbdreference_amd.build import build_generic, full_library_ready
    build_generic()                                   # shipped prebuilt in this scenario
    monkeypatch.setenv("RBD_HIPCC", "/nonexistent/hipcc")
    m = _fresh_robot("no_compiler_probe_n3", [-1, 0, 1], 4245)
    assert not full_library_ready(m)
    L = RbdLibrary(m, build=True, lazy=True, generic="auto")
    L.fn("rbd_rnea_grad", "f32")
    assert L.served_by_generic()
    assert L.wait_specialized() is L and L._bg_err is not None
    L.fn("rbd_minv", "f64")
    assert L.served_by_generic()
    L.fn("rbd_crba", "f32")                            # (round 4: served without a compiler too)
    assert L.served_by_generic()
    L.fn("rbd_minv_bpass", "f64")
    assert L.served_by_generic()
