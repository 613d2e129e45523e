"""Energy forms of pairs of fields and the energy route of the effective conductivity, on the GPU
(include/feanet_energy.h): the kernel against tests/energy_ref.py inside canary-filled buffers, the bitwise promises
(argument symmetry, u == v, batch, repeat, nontemporal stores, fields on / off), the footprint by the method of
tests/footprint.py, and the solvers' energy_forms(), effective_conductivity(route="energy") and
effective_conductivity_torch against the dense pipeline of energy_ref.py.

Field tolerance (the scheme of generic_ref.py and test_gpu_flux.py): |dens - ref| <= 2 k u S.  In
d = (sc_u sc_v + sr_u sr_v) 0.25 + (w_u w_v) (1/6) no node value passes through more than k = 5 roundings (a node
difference, the sum or difference of two of them, the product, the sum of the two products or the factor 1/6 — the
factor 0.25 is exact — and the last addition; a fused multiply-add only removes one); S is the absolute companion
(energy_ref.companions), u = 2^-24 / 2^-53, and the factor 2 covers the second-order terms and the fp64 reference's own
error.  The reference is the same expression in fp64 at the inputs the kernel reads (u, v and 1/6 as values of T).
Unlike q of fea_flux, d has products that feed additions, so -ffp-contract fuses and the bits are not numpy's.

Sums tolerance: (k u_T + 2 N 2^-53) S_sum, N = He We terms, S_sum the sum of the companions over the elements.  The
kernel adds the T values of the elements in double: every one is within k u_T S of the exact value (d(u, v) has both
signs, so nothing relative to the sum itself can be promised), and N double additions on each side add N 2^-53 S_sum."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT  # first: puts the package and the oracle on sys.path (the child process runs this file)

import energy_ref as er
import flux_ref as fx
import phase_ref as pr
from footprint import C1, C2, Geo, _same, canary
from test_energy_host import check_energy_refusals

pytestmark = pytest.mark.gpu

U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NPDT = {"f32": np.float32, "f64": np.float64}
TDT = {"f32": torch.float32, "f64": torch.float64}
K_ROUND = 5
# 3 x 3: one element row per task, one strip; 4 x 5: W - 1 no multiple of VEC; 13 x 17: a rectangle; 34 x 130 (fp64) /
# 34 x 258 (fp32): W - 2 a whole strip, the last strip holds the boundary column alone; 70 x 300: several strips,
# several row tasks with a short last one
SHAPES = {"f32": [(3, 3), (4, 5), (13, 17), (34, 258), (70, 300)],
          "f64": [(3, 3), (4, 5), (13, 17), (34, 130), (70, 300)]}
CASES = [(suf, H, W) for suf in ("f32", "f64") for H, W in SHAPES[suf]]
DPAD, PTAIL, STAIL = 3, 16, 8   # extra vectors per dens row; canary doubles behind part and sums
NS = er.NSUMS


def draw(rng, B, H, W, suf):
    """standard normal fp32 values (both kernels read the same numbers)"""
    return rng.standard_normal((B, H, W)).astype(np.float32).astype(NPDT[suf])


def draw_phase(rng, He, We):
    return (rng.random((He, We)) < 0.4).astype(np.uint8) * rng.integers(1, 256, (He, We)).astype(np.uint8)


class Call:
    """One fea_energy + fea_energy_final call on host data; every buffer is a raw allocation with canaries around the
    documented write sets, downloaded after the call.  v None: the call gets u's own buffer as v."""

    def __init__(self, suf, u, v, phase=None, fields=True, fill=0.0, byte=C1, ldp_extra=0):
        from feanet_amd import _lib
        dt = NPDT[suf]
        self.suf, self.B, (self.H, self.W) = suf, u.shape[0], u.shape[1:]
        B, H, W = self.B, self.H, self.W
        He, We = H - 1, W - 1
        esz = np.dtype(dt).itemsize
        self.geo = g = Geo(H, W, B, esz)
        self.vec = vec = 16 // esz
        self.ldd = ldd = (-(-We // vec) + DPAD) * vec
        self.per = per = int(_lib.lib().fea_energy_parts(H, W, esz))
        self.u0 = g.framed(u, fill, dt)
        self.v0 = None if v is None else g.framed(v, fill, dt)
        self.ldp = We + ldp_extra
        self.ph0 = None
        if phase is not None:
            self.ph0 = np.full(He * self.ldp + 7, 0xEE, np.uint8)
            self.ph0[(np.arange(He)[:, None] * self.ldp + np.arange(We)[None, :]).ravel()] = phase.ravel()
        self.d0 = canary(B * 3 * He * ldd + 4 * vec, dt, byte) if fields else None
        self.part0 = canary(B * NS * per + PTAIL, np.float64, byte)
        self.sums0 = canary(B * NS + STAIL, np.float64, byte)
        up = lambda a: None if a is None else torch.from_numpy(a.view(np.uint8)).cuda()
        tu, tv, tp, td, tpart, tsums = (up(a) for a in (self.u0, self.v0, self.ph0, self.d0, self.part0, self.sums0))
        ptr = lambda t: None if t is None else t.data_ptr()
        lib = _lib.lib()
        rc = getattr(lib, f"fea_energy_{suf}")(ptr(tu), ptr(tu if tv is None else tv), ptr(tp), self.ldp, ptr(td), ldd,
                                               He * ldd, 3 * He * ldd, ptr(tpart), B, H, W, g.ld, g.bs, g.bs, None)
        assert rc == 0, f"fea_energy_{suf} returned {rc}"
        rc = lib.fea_energy_final(ptr(tpart), per, ptr(tsums), B, None)
        assert rc == 0, f"fea_energy_final returned {rc}"
        torch.cuda.synchronize()
        down = lambda t, like: None if t is None else t.cpu().numpy().view(like.dtype)
        self.u1, self.v1 = down(tu, self.u0), down(tv, self.u0)
        self.ph1, self.d1 = down(tp, np.zeros(0, np.uint8)), down(td, self.u0)
        self.part1, self.sums1 = down(tpart, self.part0), down(tsums, self.sums0)
        self.dmask = None
        if fields:
            self.dmask = np.zeros(self.d0.size, bool)
            self.dmask[:B * 3 * He * ldd].reshape(B, 3, He, ldd)[..., :We] = True

    @property
    def dens(self):
        """[B, 3, He, We]"""
        B, He, We = self.B, self.H - 1, self.W - 1
        return self.d1[:B * 3 * He * self.ldd].reshape(B, 3, He, self.ldd)[..., :We]

    @property
    def part(self):
        return self.part1[:self.B * NS * self.per].reshape(self.B, NS, self.per)

    @property
    def sums(self):
        return self.sums1[:self.B * NS].reshape(self.B, NS)

    def check_footprint(self):
        """inputs unchanged; outside its write set every output still holds its canary; every element of a write set
        was stored"""
        assert _same(self.u0, self.u1).all(), "u modified"
        if self.v0 is not None:
            assert _same(self.v0, self.v1).all(), "v modified"
        if self.ph0 is not None:
            assert np.array_equal(self.ph0, self.ph1), "phase modified"
        if self.d0 is not None:
            moved = ~_same(self.d0, self.d1)
            assert not (moved & ~self.dmask).any(), "dens written outside the He x We elements (pad columns, tail)"
            assert (moved | ~self.dmask).all(), "dens element never stored"
        n = self.B * NS * self.per
        assert _same(self.part0[n:], self.part1[n:]).all(), "part written beyond B * 6 * per"
        assert not _same(self.part0[:n], self.part1[:n]).any(), "a partial slot was never stored"
        n = self.B * NS
        assert _same(self.sums0[n:], self.sums1[n:]).all(), "sums written beyond B * 6"
        assert not _same(self.sums0[:n], self.sums1[:n]).any(), "a sum was never stored"


def bits(a):
    return np.ascontiguousarray(a).view(f"u{a.dtype.itemsize}")


def same_outputs(a, b):
    return np.array_equal(bits(a.part), bits(b.part)) and np.array_equal(bits(a.sums), bits(b.sums)) and \
        (a.d0 is None or b.d0 is None or np.array_equal(bits(a.dens), bits(b.dens)))


def check_values(c, u, v, phase, suf, what):
    """dens against the fp64 reference within the field bound; sums within theirs"""
    dt = NPDT[suf]
    ref = er.element_values(u, v, dt, wide=True)
    S = er.companions(u, v, dt)
    if c.d0 is not None:
        for j, name in enumerate(er.NAMES):
            err, bound = np.abs(c.dens[:, j].astype(np.float64) - ref[name]), 2 * K_ROUND * U[suf] * S[name]
            print(f"{what} {name}: max err / bound = {(err / np.where(bound > 0, bound, 1)).max():.3g}")
            assert (err <= bound).all(), (what, name)
    want = er.sums_of(ref, phase)
    Ssum = er.sums_of(S, phase)
    N = (c.H - 1) * (c.W - 1)
    tol = (K_ROUND * U[suf] + 2 * N * 2.0 ** -53) * Ssum
    err = np.abs(c.sums - want)
    print(f"{what} sums: max err / tol = {(err / np.where(tol > 0, tol, 1)).max():.3g}")
    assert (err <= tol).all(), (what, err, tol)
    if phase is None:
        assert (c.sums[:, 1::2] == 0).all() and (c.part[:, 1::2] == 0).all(), "phase-1 sums without an image"


# ----------------------------------------------------------------------------- the kernel against energy_ref
@pytest.mark.parametrize("suf, H, W", CASES)
def test_kernel_against_reference(suf, H, W):
    """A batch of 3 pairs of random fields, without an image and with a random pitched one (non-zero bytes of any
    value count as 1), with and without the densities; fields off gives the sums of fields on; no image is the
    all-zero image."""
    rng = np.random.default_rng([H, W, len(suf)])
    u, v = draw(rng, 3, H, W, suf), draw(rng, 3, H, W, suf)
    img = draw_phase(rng, H - 1, W - 1)
    for phase, extra in ((None, 0), (img, 5)):
        what = f"{suf} {H}x{W} {'no image' if phase is None else f'image pitch +{extra}'}"
        full = Call(suf, u, v, phase, True, ldp_extra=extra)
        full.check_footprint()
        check_values(full, u, v, phase, suf, what)
        only = Call(suf, u, v, phase, False, ldp_extra=extra)
        only.check_footprint()
        assert same_outputs(only, full), (what, "sums only differ")
        if phase is None:
            assert same_outputs(Call(suf, u, v, np.zeros_like(img), True), full), (what, "all-zero image differs")


@pytest.mark.parametrize("suf, H, W", CASES)
def test_bitwise_promises(suf, H, W):
    """(u, v) and (v, u): the same uv sums and field, uu and vv swapped.  u == v, as one buffer and as two: uu == uv ==
    vv.  A pair alone gives the bits it gives inside the batch of 3, and a second run repeats them."""
    rng = np.random.default_rng([H, W, len(suf), 1])
    u, v = draw(rng, 3, H, W, suf), draw(rng, 3, H, W, suf)
    img = draw_phase(rng, H - 1, W - 1)
    a, b = Call(suf, u, v, img), Call(suf, v, u, img)
    swap = [4, 5, 2, 3, 0, 1]
    assert np.array_equal(bits(a.sums), bits(b.sums[:, swap])) and np.array_equal(bits(a.part), bits(b.part[:, swap]))
    assert np.array_equal(bits(a.dens), bits(b.dens[:, [2, 1, 0]]))
    assert same_outputs(Call(suf, u, v, img), a), "a second run differs"
    for c in (Call(suf, u, None, img), Call(suf, u, u.copy(), img)):
        c.check_footprint()
        assert np.array_equal(bits(c.sums[:, 0:2]), bits(c.sums[:, 2:4])) and \
            np.array_equal(bits(c.sums[:, 0:2]), bits(c.sums[:, 4:6]))
        assert np.array_equal(bits(c.dens[:, 0]), bits(c.dens[:, 1]))
        assert np.array_equal(bits(c.dens[:, 0]), bits(c.dens[:, 2]))
        assert np.array_equal(bits(c.sums[:, 0:2]), bits(a.sums[:, 0:2]))
        assert np.array_equal(bits(c.dens[:, 0]), bits(a.dens[:, 0]))
    for i in range(3):
        one = Call(suf, u[i:i + 1], v[i:i + 1], img)
        one.check_footprint()
        assert np.array_equal(bits(one.dens[0]), bits(a.dens[i])), (i, "dens differs from the batch's")
        assert np.array_equal(bits(one.part[0]), bits(a.part[i])) and np.array_equal(bits(one.sums[0]), bits(a.sums[i]))


# ----------------------------------------------------------------------------- footprint, nontemporal stores
FOOT = {"f32": [(3, 3), (4, 5), (34, 258)], "f64": [(3, 3), (13, 17), (34, 130)]}


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_footprint_and_padding_independence(suf):
    """Run Z (zeros in the ghost ring, the pad columns and the slack between and behind the samples of u and v, canary
    C1 in the outputs) against run P (quiet NaNs there, canary C2): the same bits on every write set, canaries
    untouched around them (dens' pad columns included), inputs unchanged.  Then one NaN node of u: exactly its own
    pair's uu and uv sums are non-finite."""
    for H, W in FOOT[suf]:
        rng = np.random.default_rng([H, W, 3])
        u, v, img = draw(rng, 3, H, W, suf), draw(rng, 3, H, W, suf), draw_phase(rng, H - 1, W - 1)
        z = Call(suf, u, v, img, True, fill=0.0, byte=C1, ldp_extra=3)
        p = Call(suf, u, v, img, True, fill=np.nan, byte=C2, ldp_extra=3)
        assert np.isnan(p.u0[~p.geo.nodes()]).all() and np.isnan(p.v0[~p.geo.nodes()]).all()
        assert not np.isnan(p.u0[p.geo.nodes()]).any()
        z.check_footprint(), p.check_footprint()
        assert same_outputs(z, p), (H, W, "a result depends on non-node storage")
        assert np.isfinite(z.sums).all()
        j, (r, c) = 1, (H - 1, W - 1)
        bad = u.copy()
        bad[j, r, c] = np.nan
        n = Call(suf, bad, v, np.zeros_like(img), True, fill=np.nan)
        assert not np.isfinite(n.sums[j, [0, 2]]).any() and np.isfinite(n.sums[j, 4]), (H, W)
        for b in (0, 2):
            assert np.isfinite(n.sums[b]).all(), (H, W, b, "leak between pairs")


def child_main(out):
    """(child process) one call with the densities on fixed data; FEANET_NT_BYTES comes from the environment"""
    rng = np.random.default_rng(11)
    res = {}
    for suf, (H, W) in (("f32", (34, 258)), ("f64", (13, 17))):
        u, v, img = draw(rng, 2, H, W, suf), draw(rng, 2, H, W, suf), draw_phase(rng, H - 1, W - 1)
        c = Call(suf, u, v, img, True)
        c.check_footprint()
        res[f"d_{suf}"], res[f"part_{suf}"], res[f"sums_{suf}"] = c.d1, c.part1, c.sums1
    np.savez(out, **res)


def test_nontemporal_stores_give_the_same_bits(tmp_path):
    """FEANET_NT_BYTES=0 (every dens streams past the caches) against a threshold no field reaches, each in a fresh
    process (the mechanism of test_gpu_flux.py): the same bytes in dens (pad columns' canaries included), the partials
    and the sums."""
    outs = []
    for name, value in (("nt", "0"), ("cached", str(1 << 40))):
        out = str(tmp_path / f"{name}.npz")
        env = dict(os.environ, FEANET_NT_BYTES=value)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=env, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(np.load(out))
    assert sorted(outs[0].files) == sorted(outs[1].files) and len(outs[0].files) == 6
    for key in outs[0].files:
        assert np.array_equal(bits(outs[0][key]), bits(outs[1][key])), key


# ----------------------------------------------------------------------------- refusals, host layer
def test_refusals():
    from feanet_amd import MultigridSolver, PCGSolver, energy_forms
    for suf, esz in (("f32", 4), ("f64", 8)):
        check_energy_refusals(suf, esz)
    x = torch.zeros(2, 1, 5, 7, device="cuda", dtype=torch.float64)
    with pytest.raises(RuntimeError, match="MI355X"):
        energy_forms(x.cpu())
    with pytest.raises(TypeError, match="float32 or float64"):
        energy_forms(x.half())
    with pytest.raises(TypeError, match="u's dtype"):
        energy_forms(x, x.float())
    with pytest.raises(TypeError, match="u's dtype"):
        energy_forms(x, x.cpu())
    with pytest.raises(ValueError, match="v has shape"):
        energy_forms(x, torch.zeros(2, 1, 7, 5, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="v has shape"):
        energy_forms(x, x[:1])
    with pytest.raises(ValueError, match="phase image is"):
        energy_forms(x, phase=np.zeros((5, 7), np.uint8))
    with pytest.raises(ValueError, match="is empty"):
        energy_forms(x[:0])
    one = MultigridSolver(16, problem="poisson", batch=1)
    with pytest.raises(ValueError, match="batch of 1"):
        one.energy_forms()
    assert one.energy_forms(pair=(0, 0)).A.shape == (1, 2, 3)
    with pytest.raises(ValueError, match="batch of 2"):
        PCGSolver(16, problem="poisson", batch=2).energy_forms(pair=(0, 2))


def test_host_layer_energy_forms():
    """energy_forms on plain tensors: A [B, 2, 3] in phase-major order, the padded allocation's view, v = None."""
    from feanet_amd import energy_forms
    rng = np.random.default_rng(5)
    for suf, (H, W) in (("f64", (13, 17)), ("f32", (4, 5)), ("f64", (34, 130))):
        u, v, img = draw(rng, 2, H, W, suf), draw(rng, 2, H, W, suf), draw_phase(rng, H - 1, W - 1)
        tu, tv = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
        res = energy_forms(tu.reshape(2, 1, H, W), tv, torch.from_numpy(img != 0).cuda())
        ref = Call(suf, u, v, img, True)
        assert res.A.shape == (2, 2, 3) and res.A.dtype == torch.float64 and res.A.is_cuda
        assert res.density.shape == (2, 3, H - 1, W - 1) and res.density.dtype == TDT[suf]
        assert np.array_equal(res.A.cpu().numpy(), ref.sums.reshape(2, 3, 2).transpose(0, 2, 1))
        assert np.array_equal(bits(res.density.cpu().numpy()), bits(ref.dens))
        off = energy_forms(tu, tv, img != 0, fields=False)
        assert off.density is None and torch.equal(off.A, res.A)
        same = energy_forms(tu, phase=img != 0)
        assert torch.equal(same.A[..., 0], same.A[..., 1]) and torch.equal(same.A[..., 0], same.A[..., 2])
        assert torch.equal(same.A[..., 0], res.A[..., 0])
        none = energy_forms(tu, tv)
        assert bool((none.A[:, 1] == 0).all())


# ----------------------------------------------------------------------------- the solvers
RTOL = 1e-10
# (image, m, n, prop, mixed): the allowance was first measured on the CPU, with phase_ref.numpy_pcg iterates stopped at
# the same rtol, against the dense reference on the same float32 table: |K_E - ref| / max|K_E| = 1.8e-16 (six discs,
# fp64 and mixed), 3.8e-16 (off-centre disc, fp64) and 8.8e-14 (off-centre disc, mixed).  The tests allow
# 100 rtol = 1e-8, the margin of test_gpu_flux.py's solver tests: the stopping rule bounds the FLUX route by a factor
# of rtol that test computes (residual_bound, at most 6.3 on these images), and the energy route's error is the square
# of the same field error, so the margin that holds the flux route holds this one with room to spare.
SOLVES = [("six_discs", 32, 48, (1, 20), False), ("six_discs", 32, 48, (1, 20), True),
          ("offcentre_disc", 64, 64, (1, 1000), False)]


def defects(name, m, n, prop):
    """Hill and symmetry defect of the dense flux pipeline on this image and float32 table"""
    r = fx.homogenize_image(name, m, n, prop)
    return float(r["hill"].max()), float(r["sym"])


@pytest.mark.parametrize("name, m, n, prop, mixed", SOLVES, ids=lambda v: str(v).replace(" ", ""))
def test_effective_conductivity_energy_route(name, m, n, prop, mixed):
    """PCG against the dense reference of energy_ref.py on the same float32 table: K_E and dK_dprop within 100 rtol,
    K_eff exactly symmetric and equal to sum_p k_p dK_dprop[p], the sensitivity field sums to dK_dprop, the flux
    route from the same solve is test_gpu_flux.py's, and route_gap lies within the Hill and symmetry defects the dense
    flux pipeline shows on this image and contrast (K_E - K_flux is the Hill defect on the diagonal and half the sum
    of the two mixed ones off it; at 64 x 64 and (1, 1000) they are 1.2e-4 and 1.1e-4, DESIGN §16: they grow with
    the grid)."""
    from feanet_amd import effective_conductivity
    ref = er.homogenize_image(name, m, n, prop)
    kw = dict(precond_dtype=torch.float32) if mixed else {}
    res = effective_conductivity(pr.image(name, m, n), prop=prop, rtol=RTOL, route="energy", coarsen="stiff", **kw)
    assert res.flags.tolist() == [1, 1] and res.converged, f"flags {res.flags}, iterations {res.iterations}"
    scale = np.abs(ref["K_E"]).max()
    err = np.abs(res.K_eff - ref["K_E"]).max() / scale
    hill, sym = defects(name, m, n, prop)
    print(f"{m}x{n} {name} {prop}{' mixed' if mixed else ''}: iterations {res.iterations.tolist()}, K_E error "
          f"{err:.2e} of max|K_E| (allowed {100 * RTOL:.0e}), route gap {res.route_gap:.2e} (dense {ref['gap']:.2e}, "
          f"Hill {hill:.2e}, symmetry {sym:.2e})")
    assert res.K_eff.shape == (2, 2) and res.K_eff.dtype == np.float64 and res.dK_dprop.shape == (2, 2, 2)
    assert err <= 100 * RTOL
    assert res.K_eff[0, 1] == res.K_eff[1, 0]
    assert np.array_equal(res.dK_dprop, res.dK_dprop.transpose(0, 2, 1))
    k0, k1 = er.coefficients(prop, False)
    assert np.array_equal(res.K_eff, k0 * res.dK_dprop[0] + k1 * res.dK_dprop[1])
    assert np.abs(res.dK_dprop - ref["dK"]).max() <= 100 * RTOL * np.abs(ref["dK"]).max()
    assert np.abs(res.K_eff_flux - ref["K_flux"]).max() <= 100 * RTOL * scale
    assert res.route_gap <= hill + sym + 200 * RTOL
    # the sensitivity: [3, m, n] in the solver's dtype, on the device; its sums over the phases are dK_dprop
    s = res.sensitivity
    assert s.shape == (3, m, n) and s.dtype == torch.float64 and s.is_cuda
    img = pr.image(name, m, n) != 0
    sn = s.cpu().numpy()
    got = np.array([[sn[j][img == p].sum() for j in range(3)] for p in (False, True)])
    want = res.dK_dprop[:, [0, 0, 1], [0, 1, 1]]
    assert np.abs(got - want).max() <= m * n * 2.0 ** -52 * np.abs(sn).sum() + 1e-300
    off = effective_conductivity(pr.image(name, m, n), prop=prop, rtol=RTOL, route="energy", fields=False, **kw)
    assert off.sensitivity is None and np.array_equal(off.K_eff, res.K_eff)


@pytest.mark.parametrize("value", [0, 1])
def test_homogeneous_image(value):
    """K_E = k I, dK_dprop = I on the phase present and 0 on the other, within the field bound of d on the linear
    load cases (h = 1/32 is a power of two: no iteration, and the mixed form is exactly 0)."""
    from feanet_amd import effective_conductivity
    m = n = 64
    prop = (1, 20)
    res = effective_conductivity(np.full((m, n), value, np.uint8), prop=prop, route="energy")
    assert res.flags.tolist() == [1, 1] and res.iterations.tolist() == [0, 0]
    k = float(prop[value])
    x = fx.load_cases(m, n, 2.0)
    S = er.companions(x[0:1], x[1:2], np.float64)
    vol = m * n * (2.0 / n) ** 2
    tol = 2 * (K_ROUND + 1) * 2.0 ** -53 * max(S[nm].sum() for nm in er.NAMES) / vol   # (+ 1: the division by |V|)
    assert np.abs(res.dK_dprop[value] - np.eye(2)).max() <= tol
    assert (res.dK_dprop[1 - value] == 0).all() and res.dK_dprop[value][0, 1] == 0
    assert np.abs(res.K_eff - k * np.eye(2)).max() <= k * tol and res.route_gap <= 2 * tol
    assert np.array_equal(res.K_eff_flux, k * np.eye(2))


LOOSE = 1e-3


def test_second_order_on_the_device():
    """six discs, 32 x 48, (1, 20), fp64 PCG stopped at rtol = 1e-3.  The loose rtol is chosen on the CPU: for the
    numpy PCG's iterate x = u + dv the diagonal of K_E(x) - K_E(u) splits into the quadratic term a(dv, dv) / |V| and
    the term 2 a(u, dv) / |V|, which the exact K would make zero and the float32 table leaves at its rounding level;
    at 1e-3 the first is 530 and 1500 times the second (asserted below to be at least 100 times).  Then on the device
    diag(K_E(loose) - K_E(1e-10)) >= 0 and the energy route's error is no larger than the flux route's of the same
    iterate.  Measured ratio flux error / energy error on the CPU: 50; the device's is printed."""
    from feanet_amd import effective_conductivity
    name, m, n, prop = "six_discs", 32, 48, (1, 20)
    img = pr.image(name, m, n)
    ref = er.homogenize_image(name, m, n, prop)
    k0, k1 = er.coefficients(prop, False)
    x, _ = er.pcg_iterates(img, prop, LOOSE)
    quad = np.diag(er.routes(x - ref["u"], img, k0, k1)["K_E"])
    lin = np.diag(er.routes(x, img, k0, k1)["K_E"] - ref["K_E"]) - quad
    print(f"CPU at rtol {LOOSE}: quadratic term {quad}, float32-table term {lin}")
    assert (quad >= 100 * np.abs(lin)).all()
    tight = effective_conductivity(img, prop=prop, rtol=RTOL, route="energy", fields=False)
    loose = effective_conductivity(img, prop=prop, rtol=LOOSE, route="energy", fields=False)
    assert tight.converged and loose.converged and (loose.iterations < tight.iterations).all()
    d = np.diag(loose.K_eff - tight.K_eff)
    eE = np.abs(loose.K_eff - tight.K_eff).max()
    eF = np.abs(loose.K_eff_flux - tight.K_eff_flux).max()
    print(f"device at rtol {LOOSE}: iterations {loose.iterations.tolist()} against {tight.iterations.tolist()}, "
          f"diag(K_E(loose) - K_E(tight)) {d}, energy-route error {eE:.3e}, flux-route error {eF:.3e}, "
          f"ratio {eF / eE:.1f}")
    assert (d >= 0).all()
    assert eE <= eF


@pytest.mark.parametrize("T", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_multigrid_solver_energy_forms_reads_the_current_iterate(T):
    """MultigridSolver on an image, batch 2, after joined cycles (the iterate rests mid-cycle): energy_forms() is the
    kernel on the fields solution() returns, with the solver's image; it changes after vcycle()."""
    from feanet_amd import MultigridSolver
    suf = "f32" if T == torch.float32 else "f64"
    m, n, B = 32, 48, 2
    img = pr.six_discs(m, n)
    rng = np.random.default_rng(9)
    s = MultigridSolver(n, rows=m, problem="interface", dtype=T, batch=B, prop=(1, 20), phase=img, coarsen="stiff")
    s.set_boundary(torch.from_numpy(rng.standard_normal((B, 1, m + 1, n + 1))).cuda().to(T))
    s.set_rhs(f=torch.from_numpy(rng.standard_normal((B, 1, m + 1, n + 1))).cuda().to(T))
    s.load()
    s.vcycle(3)
    res = s.energy_forms()
    x = s.solution().cpu().numpy()[:, 0]
    ref = Call(suf, x[0:1], x[1:2], img, True)
    assert res.A.shape == (1, 2, 3) and res.density.shape == (1, 3, m, n) and res.density.dtype == T
    assert np.array_equal(res.A.cpu().numpy()[0], ref.sums.reshape(3, 2).T)
    assert np.array_equal(bits(res.density.cpu().numpy()), bits(ref.dens))
    flipped = s.energy_forms(pair=(1, 0), fields=False)
    assert flipped.density is None and torch.equal(flipped.A, res.A[..., [2, 1, 0]])
    own = s.energy_forms(pair=(1, 1), fields=False)
    assert torch.equal(own.A[..., 0], res.A[..., 2]) and torch.equal(own.A[..., 1], res.A[..., 2])
    s.vcycle()
    assert not torch.equal(s.energy_forms(fields=False).A, res.A)


def test_pcg_solver_energy_forms_mixed_reads_the_fp64_iterate():
    from feanet_amd import PCGSolver
    m, n = 32, 48
    img = pr.six_discs(m, n)
    s = PCGSolver(n, rows=m, problem="interface", batch=2, prop=(1, 20), phase=img, coarsen="stiff",
                  precond_dtype=torch.float32)
    u0 = torch.from_numpy(fx.load_cases(m, n, 2.0)).cuda().reshape(2, 1, m + 1, n + 1)
    bc = u0.clone()
    bc[..., 1:-1, 1:-1] = 0
    s.solve(u0=u0, f=torch.zeros_like(u0), rtol=1e-6, max_iters=50, bc_value=bc)
    res = s.energy_forms()
    assert res.density.dtype == torch.float64
    x = s.solution().cpu().numpy()[:, 0]
    assert x.dtype == np.float64
    ref = Call("f64", x[0:1], x[1:2], img, True)
    assert np.array_equal(res.A.cpu().numpy()[0], ref.sums.reshape(3, 2).T)
    assert np.array_equal(bits(res.density.cpu().numpy()), bits(ref.dens))


def test_effective_conductivity_torch_backward():
    """Backward against central differences in k1 with steps that are exact in float32, 20 +/- 0.25, six discs at
    32 x 32.  The tolerance is the truncation error of that difference, measured with dense CPU solves on the same
    float32 table (|difference quotient - A_1 / |V|| = 5.8e-07 here, 1e-4 of dK/dk1; computed below, and allowed
    twice), plus what three solves stopped at rtol add: 2 * 100 rtol max|K_E| / 0.5 for the quotient and 100 rtol
    max|dK/dk1| for the derivative."""
    from feanet_amd import effective_conductivity_torch
    m = n = 32
    img = pr.six_discs(m, n)
    ref = er.homogenize_image("six_discs", m, n, (1, 20))
    cd, _ = er.central_difference(img, (1, 20), exact=False, step=0.25)
    trunc = np.abs(cd - ref["dK"][1]).max()
    tol = 2 * trunc + 2 * 100 * RTOL * np.abs(ref["K_E"]).max() / 0.5 + 100 * RTOL * np.abs(ref["dK"][1]).max()
    prop = torch.tensor([1.0, 20.0], dtype=torch.float64, device="cuda", requires_grad=True)
    K = effective_conductivity_torch(img, prop, rtol=RTOL)
    assert K.shape == (2, 2) and K.dtype == torch.float64 and K.is_cuda and K.requires_grad
    assert np.abs(K.detach().cpu().numpy() - ref["K_E"]).max() <= 100 * RTOL * np.abs(ref["K_E"]).max()
    hi = effective_conductivity_torch(img, torch.tensor([1.0, 20.25]), rtol=RTOL)
    lo = effective_conductivity_torch(img, torch.tensor([1.0, 19.75]), rtol=RTOL)
    assert not hi.is_cuda and not hi.requires_grad
    quotient = ((hi - lo) / 0.5).numpy()
    for i, j in ((0, 0), (0, 1), (1, 1)):
        g, = torch.autograd.grad(K[i, j], prop, retain_graph=True)
        g = g.cpu().numpy()
        print(f"dK[{i}, {j}] / dprop = {g}, difference quotient in k1 {quotient[i, j]:.9e} (truncation {trunc:.2e}, "
              f"allowed {tol:.2e})")
        assert abs(g[1] - quotient[i, j]) <= tol
        assert abs(g[0] - ref["dK"][0][i, j]) <= 100 * RTOL * np.abs(ref["dK"][0]).max()
    # a weighted sum contracts the incoming gradient with dK_dprop; the gradient comes back in prop's dtype
    w = torch.tensor([[1.0, -2.0], [0.5, 3.0]], dtype=torch.float64, device="cuda")
    p32 = torch.tensor([1.0, 20.0], requires_grad=True)
    (effective_conductivity_torch(img, p32, rtol=RTOL) * w.cpu()).sum().backward()
    want = (ref["dK"] * w.cpu().numpy()).sum((1, 2))
    assert p32.grad.dtype == torch.float32 and np.abs(p32.grad.numpy() - want).max() <= 2.0 ** -22 * np.abs(want).max()


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child_main(sys.argv[2])
