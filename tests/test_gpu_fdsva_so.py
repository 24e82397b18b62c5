"""Second-order forward-dynamics derivatives on the GPU (rbd_fdsva_so through RBDReference.fdsva_so) against the numpy
restatement (tests/fdso_oracle.py) and, where the two are meant to agree, the fixtures of the real reference
(tests/golden/fdso_*.npz).  Libraries come from build()."""
import ctypes
import os

import numpy as np
import pytest

from conftest import make_robot
from fdso_oracle import FDSOOracle, contract
from oracle import rbd_oracle as orc
from so_oracle import SO_ROBOTS

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::PendingDeprecationWarning")]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("daba_dqdq", "daba_dvdq", "daba_dvdv", "daba_dtdq")
TOL64 = 1e-9                # the project's tol_fd for everything multiplied by Minv (eps64 * cond(H) <= 1e-11 here)
EPS32 = 2.0 ** -24          # unit round-off of float32
COND_SLACK = 8.0            # as tests/test_gpu_parity.py: rounding errors of an O(10)-operation chain, all adding up
_RBD = {}


def _rbd(name):
    from rbdreference_amd import RBDReference
    if name not in _RBD:
        _RBD[name] = RBDReference(make_robot(name), build=False)
    return _RBD[name]


def _torch_dtype(dt):
    import torch
    return torch.float64 if dt == "f64" else torch.float32


def _inputs(q, qd, u, dt):
    """Device tensors, and the same values in fp64 for the oracle (the fp32 rounding of the inputs is not an error)."""
    import torch
    ts = [torch.tensor(x, device="cuda:0", dtype=_torch_dtype(dt)) for x in (q, qd, u)]
    return ts, [t.double().cpu().numpy() for t in ts]


def _row_err(x, r):
    """Normwise error per row (configuration) and output: [B, 4]."""
    x = np.asarray(x, dtype=np.float64).reshape(r.shape[0], r.shape[1], -1)
    r = r.reshape(x.shape)
    d = np.abs(x - r).max(-1)
    s = np.abs(r).max(-1)
    return d / np.where(s > 0, s, 1.0)


def _stack(outs):
    import torch
    return torch.stack([o.double() for o in outs], 1).cpu().numpy()


def _cond_rows(robot, q):
    """2-norm condition number of every row's joint-space inertia, from the oracle's crba."""
    H = orc.crba(orc.model_from_robot(robot), np.asarray(q, dtype=np.float64))
    return np.array([np.linalg.cond(h) for h in H])


def _own_fp32_composition(rbd, tq, tqd, tu, grav):
    """fp64 contract(...) of this package's own fp32 minv, forward_dynamics_grad and second_order_idsva_parallel on the
    same rows (qdd is the one the forward_dynamics_grad entry point returns, as inside rbd_fdsva_so)."""
    qdd, d, _, _ = rbd._fd(tq, tqd, tu, grav, True)
    n = rbd.n
    Mi = rbd.minv(tq)
    so = rbd.second_order_idsva_parallel(tq, tqd, qdd, grav)
    f = lambda t: t.double().cpu().numpy()      # noqa: E731
    return np.stack(contract(f(Mi), f(d[..., :n]), f(d[..., n:]), *(f(x) for x in so)), 1)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", SO_ROBOTS)
def test_matches_oracle_and_reference_fixtures(name, dt):
    g = dict(np.load(os.path.join(GOLDEN, f"fdso_{name}.npz")))
    rbd = _rbd(name)
    grav = float(g["gravity"])
    (tq, tqd, tu), (q, qd, u) = _inputs(g["q"], g["qd"], g["u"], dt)
    outs = rbd.fdsva_so(tq, tqd, tu, grav)
    got = _stack(outs)
    ref = np.stack(FDSOOracle(rbd.robot)(q, qd, u, grav), 1)
    e = _row_err(got, ref)
    base = outs[0].untyped_storage().data_ptr()
    assert all(o.untyped_storage().data_ptr() == base for o in outs)   # views of one [B, 4, n, n, n] buffer
    if dt == "f64":
        print(f"fdsva_so {name} f64: vs oracle {e.max(0)}")
        assert e.max() <= TOL64, (name, dt, e.max(0))
        fx = np.stack([g[k] for k in KEYS], 1)                        # the reference itself (its inputs are fp64)
        ef = _row_err(got, fx)
        print(f"fdsva_so {name} f64: vs reference fixtures {ef.max(0)}")
        cols = slice(0, 4) if bool(g["unbranched"]) else slice(1, 4)   # decision 1: daba_dqdq differs on branched robots
        assert ef[:, cols].max() <= TOL64, (name, ef.max(0))
        return
    cond = _cond_rows(rbd.robot, q)
    own = _own_fp32_composition(rbd, tq, tqd, tu, grav)
    ea = _row_err(got, own) / (EPS32 * cond)[:, None]
    eb = e / (EPS32 * cond)[:, None]
    print(f"fdsva_so {name} f32: cond(H) max {cond.max():.3g}; err / (eps32 cond): vs own fp32 composition "
          f"{ea.max(0)} (bound {COND_SLACK}), vs fp64 oracle {eb.max(0)} (bound {2 * COND_SLACK}); "
          f"abs normwise vs oracle {e.max(0)}")
    assert ea.max() <= COND_SLACK, (name, "vs own fp32 composition", ea.max(0))
    assert eb.max() <= 2 * COND_SLACK, (name, "vs fp64 oracle", eb.max(0))


def test_single_configuration_returns_the_reference_types():
    import torch
    g = dict(np.load(os.path.join(GOLDEN, "fdso_random_prismatic_n6.npz")))
    rbd = _rbd("random_prismatic_n6")
    n = rbd.n
    outs = rbd.fdsva_so(g["q"][0], g["qd"][0], g["u"][0])
    assert len(outs) == 4
    ref = FDSOOracle(rbd.robot)(g["q"][0], g["qd"][0], g["u"][0])
    for x, r in zip(outs, ref):
        assert type(x) is np.ndarray and x.dtype == np.float64 and x.shape == (n, n, n)
        assert np.abs(x - r).max() <= TOL64 * np.abs(r).max()
    t = [torch.tensor(x[0], device="cuda:0") for x in (g["q"], g["qd"], g["u"])]
    outs = rbd.fdsva_so(*t)
    assert all(isinstance(x, torch.Tensor) and x.shape == (n, n, n) and x.dtype == torch.float64 for x in outs)
    outs = rbd.fdsva_so(*(torch.stack([x, x]) for x in t))
    base = outs[0].untyped_storage().data_ptr()
    assert all(o.shape == (2, n, n, n) and o.untyped_storage().data_ptr() == base for o in outs)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("name,B", [("iiwa_like", 65537), ("quadruped_like", 16385), ("atlas_like", 1025)])
def test_ragged_full_sizes_sampled_rows_guard_tail_and_workspace(name, B, dt):
    """Big batches whose size is not a multiple of a block's configurations, through ctypes into a buffer with a guard
    tail and a workspace of exactly rbd_fdsva_so_workspace_bytes: sampled rows (first and last included) match the
    oracle, the guard is untouched; one byte less of workspace is refused before any launch."""
    import torch
    from rbdreference_amd._lib import RBD_ERR_ARG
    rbd = _rbd(name)
    n = rbd.n
    rng = np.random.default_rng(B)
    tdt = _torch_dtype(dt)
    esz = 4 if dt == "f32" else 8
    q = torch.tensor(rng.uniform(-np.pi, np.pi, (B, n)), device="cuda:0", dtype=tdt)
    qd = torch.tensor(rng.uniform(-1, 1, (B, n)), device="cuda:0", dtype=tdt)
    u = torch.tensor(rng.uniform(-5, 5, (B, n)), device="cuda:0", dtype=tdt)
    per = 4 * n ** 3
    guard = 4096
    buf = torch.full((B * per + guard,), 12345.0, device="cuda:0", dtype=tdt)
    lib = rbd._lib.resolve("rbd_fdsva_so", dt)
    fn = getattr(lib, f"rbd_fdsva_so_{dt}")
    wsb = int(lib.rbd_fdsva_so_workspace_bytes(B, esz))
    assert wsb >= B * (per + 3 * n * n + n) * esz
    ws = torch.full((wsb + guard,), 0x5A, device="cuda:0", dtype=torch.uint8)
    st = torch.cuda.current_stream().cuda_stream
    args = (q.data_ptr(), qd.data_ptr(), u.data_ptr(), -9.81, B, buf.data_ptr(), ws.data_ptr())
    assert fn(*args, wsb - 1, st) == RBD_ERR_ARG
    assert b"workspace" in lib.rbd_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 12345.0).all()) and bool((ws == 0x5A).all())       # refused before any launch
    rbd._lib.check(fn(*args, wsb, st))
    torch.cuda.synchronize()
    assert bool((buf[B * per:] == 12345.0).all()) and bool((ws[wsb:] == 0x5A).all())
    rows = np.unique(np.r_[0, 1, B - 2, B - 1, rng.integers(0, B, 12)])
    trows = torch.tensor(rows, device="cuda:0")
    got = buf[: B * per].view(B, 4, n, n, n)[trows].double().cpu().numpy()
    xs = [x[rows].double().cpu().numpy() for x in (q, qd, u)]
    ref = np.stack(FDSOOracle(rbd.robot)(*xs), 1)
    e = _row_err(got, ref)
    if dt == "f64":
        print(f"fdsva_so ragged {name} B={B} f64: {e.max(0)}")
        assert e.max() <= TOL64, (name, dt, e.max(0))
    else:
        cond = _cond_rows(rbd.robot, xs[0])
        own = _own_fp32_composition(rbd, q[trows], qd[trows], u[trows], -9.81)
        ea = _row_err(got, own) / (EPS32 * cond)[:, None]
        eb = e / (EPS32 * cond)[:, None]
        print(f"fdsva_so ragged {name} B={B} f32: err / (eps32 cond) vs own {ea.max(0)}, vs oracle {eb.max(0)}")
        assert ea.max() <= COND_SLACK, (name, ea.max(0))
        assert eb.max() <= 2 * COND_SLACK, (name, eb.max(0))


@pytest.mark.parametrize("grav", [-3.7, 0.0])
def test_other_gravity(grav):
    """Decision 3: the given gravity in every stage."""
    for name in ("atlas_like", "random_prismatic_n6"):
        rbd = _rbd(name)
        rng = np.random.default_rng(7)
        x = [rng.uniform(-2, 2, (33, rbd.n)) for _ in range(3)]
        for dt in ("f64", "f32"):
            t, xs = _inputs(*x, dt)
            got = _stack(rbd.fdsva_so(*t, GRAVITY=grav))
            ref = np.stack(FDSOOracle(rbd.robot)(*xs, GRAVITY=grav), 1)
            e = _row_err(got, ref)
            if dt == "f64":
                assert e.max() <= TOL64, (name, dt, grav, e.max(0))
            else:
                eb = e / (EPS32 * _cond_rows(rbd.robot, xs[0]))[:, None]
                print(f"fdsva_so gravity {grav} {name} f32: err / (eps32 cond) vs oracle {eb.max(0)}")
                assert eb.max() <= 2 * COND_SLACK, (name, grav, eb.max(0))


@pytest.mark.parametrize("name", ["atlas_like", "random_prismatic_n6", "random_forest_n8"])
def test_fp64_derivatives_of_the_gpu_minv_and_forward_dynamics_grad_and_symmetries(name):
    """On the GPU itself: daba_dtdq against central differences of minv, daba_dvdq against central differences of
    forward_dynamics_grad's qdd_dqd; the symmetries of daba_dqdq, daba_dvdv (in j, k) and daba_dtdq (in i, j)."""
    import torch
    rbd = _rbd(name)
    n = rbd.n
    rng = np.random.default_rng(11)
    q, qd, u = (torch.tensor(rng.uniform(-2, 2, n), device="cuda:0", dtype=torch.float64) for _ in range(3))
    dqq, dvq, dvv, dtq = rbd.fdsva_so(q, qd, u)
    h = 1e-6
    E = torch.eye(n, device="cuda:0", dtype=torch.float64)
    Q = torch.cat([q + h * E, q - h * E])
    Mi = rbd.minv(Q)
    fd_M = ((Mi[:n] - Mi[n:]) / (2 * h)).permute(1, 2, 0)
    assert float((dtq - fd_M).abs().max() / dtq.abs().max()) <= 1e-6
    _, b = rbd.forward_dynamics_grad(Q, qd.expand(2 * n, n).contiguous(), u.expand(2 * n, n).contiguous())
    fd_vq = ((b[:n] - b[n:]) / (2 * h)).permute(1, 2, 0)
    assert float((dvq - fd_vq).abs().max() / dvq.abs().max()) <= 1e-6
    for x, perm in ((dqq, (0, 2, 1)), (dvv, (0, 2, 1)), (dtq, (1, 0, 2))):
        assert float((x - x.permute(*perm)).abs().max() / x.abs().max()) <= 1e-12


def test_nan_row_stays_in_its_row():
    import torch
    rbd = _rbd("atlas_like")
    rng = np.random.default_rng(4)
    x = [rng.uniform(-2, 2, (40, 30)) for _ in range(3)]
    bad = [a.copy() for a in x]
    bad[0][17, 5] = np.nan
    for dt in (torch.float32, torch.float64):
        clean = rbd.fdsva_so(*(torch.tensor(a, device="cuda:0", dtype=dt) for a in x))
        dirty = rbd.fdsva_so(*(torch.tensor(a, device="cuda:0", dtype=dt) for a in bad))
        torch.cuda.synchronize()
        keep = torch.tensor(np.setdiff1d(np.arange(40), [17]), device="cuda:0")
        for c, d in zip(clean, dirty):
            assert torch.equal(c[keep], d[keep])
        assert any(bool(torch.isnan(d[17]).any()) for d in dirty)
    rbd = _rbd("iiwa_like")                         # several configurations share a block here
    x = [rng.uniform(-2, 2, (40, 7)) for _ in range(3)]
    bad = [a.copy() for a in x]
    bad[2][17, 3] = np.nan
    clean = rbd.fdsva_so(*(torch.tensor(a, device="cuda:0", dtype=torch.float32) for a in x))
    dirty = rbd.fdsva_so(*(torch.tensor(a, device="cuda:0", dtype=torch.float32) for a in bad))
    keep = torch.tensor(np.setdiff1d(np.arange(40), [17]), device="cuda:0")
    for c, d in zip(clean, dirty):
        assert torch.equal(c[keep], d[keep])
    assert bool(torch.isnan(dirty[0][17]).any())


def test_capi_rejects_bad_arguments_before_any_launch():
    from rbdreference_amd._lib import RBD_ERR_ARG
    rbd = _rbd("iiwa_like")
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below is refused first
    for sfx, esz in (("f32", 4), ("f64", 8)):
        lib = rbd._lib.resolve("rbd_fdsva_so", sfx)
        fn = getattr(lib, f"rbd_fdsva_so_{sfx}")
        wsb = int(lib.rbd_fdsva_so_workspace_bytes(4, esz))
        assert wsb > 0 and wsb % 16 == 0
        for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
            assert fn(*args, -9.81, 4, fake, fake, wsb, None) == RBD_ERR_ARG
        assert fn(fake, fake, fake, -9.81, 4, None, fake, wsb, None) == RBD_ERR_ARG
        assert b"must be non-null" in lib.rbd_last_error()
        assert fn(fake, fake, fake, -9.81, -1, fake, fake, wsb, None) == RBD_ERR_ARG
        assert b"B < 0" in lib.rbd_last_error()
        assert fn(fake, fake, fake, -9.81, 2 ** 62, fake, fake, wsb, None) == RBD_ERR_ARG
        assert b"B too large" in lib.rbd_last_error()
        assert fn(fake, fake, fake, -9.81, 4, fake, None, wsb, None) == RBD_ERR_ARG
        assert fn(fake, fake, fake, -9.81, 4, fake, fake, wsb - 1, None) == RBD_ERR_ARG
        assert b"workspace" in lib.rbd_last_error()
        assert fn(None, None, None, -9.81, 0, None, None, 0, None) == 0
        assert int(lib.rbd_fdsva_so_workspace_bytes(0, esz)) == 0 and int(lib.rbd_fdsva_so_workspace_bytes(4, 2)) == 0


def test_floating_base_library_exports_an_unsupported_stub():
    from rbdreference_amd import RBDReference
    from rbdreference_amd._lib import RBD_ERR_UNSUPPORTED
    from rbdreference_amd.robot import floating_quadruped_like
    rbd = RBDReference(floating_quadruped_like(), build=False)
    fake = ctypes.c_void_p(4096)
    for sfx in ("f32", "f64"):
        fn = rbd._lib.fn("rbd_fdsva_so", sfx)
        assert fn(fake, fake, fake, -9.81, 4, fake, fake, 1 << 20, None) == RBD_ERR_UNSUPPORTED
    assert int(rbd._lib.lib.rbd_fdsva_so_workspace_bytes(4, 8)) == 0
    with pytest.raises(NotImplementedError):
        rbd.fdsva_so(np.zeros(rbd.nv), np.zeros(rbd.nv), np.zeros(rbd.nv))


def test_first_call_of_a_never_built_robot_goes_through_the_fdso_family_library(monkeypatch):
    """The robot's full library is held back (its background build waits until the end of the test), as on a first use:
    the call is answered by the small `fdso` family library (build.FAMILIES), built on demand."""
    import threading
    import torch
    from rbdreference_amd import RBDReference, _lib
    from rbdreference_amd.build import family_lib_path
    from rbdreference_amd.robot import random_tree
    release = threading.Event()

    def held_back_full_build(model):
        release.wait(300)
        raise RuntimeError("full library held back by the test")
    monkeypatch.setattr(_lib, "build_model", held_back_full_build)
    robot = random_tree([-1, 0, 1, 1], seed=4323, prismatic_every=3, name="fdso_first_use_n4")
    try:
        rbd = RBDReference(robot, generic="never")
        x = [torch.rand((100, 4), device="cuda:0", dtype=torch.float64) for _ in range(3)]
        outs = rbd.fdsva_so(*x)
        lib = rbd._lib._tls.lib
        assert rbd._lib._full is None and lib._name == family_lib_path(rbd.model, "fdso", "f64")
        ref = np.stack(FDSOOracle(robot)(*(t.cpu().numpy() for t in x)), 1)
        assert _row_err(_stack(outs), ref).max() <= TOL64
    finally:
        release.set()
