"""Element flux fields, their sums and the effective conductivity, on the GPU (include/feanet_flux.h): the kernel
against tests/flux_ref.py inside canary-filled buffers, the bitwise promises (batch, task height, nontemporal stores,
fields on / off), the footprint by the method of tests/footprint.py, and the solvers' flux() and
effective_conductivity() against the dense pipeline of flux_ref.py.

Field tolerance (generic_ref.py): |q - ref| <= 2 (n + m) u S.  q_r = -k ((c - a) + (d - b)) i2h is a sum of n = 4
terms, each a product of m = 3 factors (k, a node value, i2h); S = k (|a| + |b| + |c| + |d|) i2h, u = 2^-24 / 2^-53.
The reference is the same expression in fp64 at the inputs the kernel reads (u, k and i2h as values of T).  No
product of these expressions feeds an addition, so -ffp-contract has nothing to fuse and q is also the same BITS as the
expressions evaluated by numpy in T; the test asserts both.

Sums tolerance: u_T |ref| + 2 N 2^-53 S, N = He We terms, S the sum of the companions.  The kernel adds the T values
of the elements in double; the reference adds numpy's T values of the same expressions in double, so for q and g the
terms are the same bits and only the order of N double additions differs (N 2^-53 S each side).  The energy's terms
may differ by the fused multiply-adds of (sc sc + sr sr) 0.25 + w w / 6: they are positive, each within a few u_T of
numpy's, with signs that do not add up over N terms, which is what the first term allows."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT  # first: puts the package and the oracle on sys.path (the child process runs this file)

import flux_ref as fx
import phase_ref as pr
from footprint import C1, C2, SLACK, Geo, _same, canary
from test_flux_host import HILL_BOUND

pytestmark = pytest.mark.gpu

U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NPDT = {"f32": np.float32, "f64": np.float64}
TDT = {"f32": torch.float32, "f64": torch.float64}
N_TERMS, M_FACTORS = 4, 3       # q = -k ((c - a) + (d - b)) i2h
SHAPES = [(3, 3), (4, 6), (5, 130), (9, 131), (34, 258), (7, 259), (66, 515)]
K0, K1, HSTEP = 1.0, 20.0, 0.03125
QPAD, PTAIL, STAIL = 3, 16, 8   # extra vectors per q row; canary doubles behind part and sums


def draw_u(rng, B, H, W, suf):
    """standard normal fp32 values (both kernels read the same numbers)"""
    return rng.standard_normal((B, H, W)).astype(np.float32).astype(NPDT[suf])


def draw_phase(rng, He, We):
    return (rng.random((He, We)) < 0.4).astype(np.uint8) * rng.integers(1, 256, (He, We)).astype(np.uint8)


class Call:
    """One fea_flux + fea_flux_final call on host data; every buffer is a raw allocation with canaries around the
    documented write sets, downloaded after the call."""

    def __init__(self, suf, nodes, phase=None, fields=True, fill=0.0, byte=C1, ldp_extra=0, k=(K0, K1), h=HSTEP):
        from feanet_amd import _lib
        dt = NPDT[suf]
        self.suf, self.B, (self.H, self.W) = suf, nodes.shape[0], nodes.shape[1:]
        B, H, W = self.B, self.H, self.W
        He, We = H - 1, W - 1
        esz = np.dtype(dt).itemsize
        self.geo = g = Geo(H, W, B, esz)
        self.vec = vec = 16 // esz
        self.ldq = ldq = (-(-We // vec) + QPAD) * vec
        self.per = per = int(_lib.lib().fea_flux_parts(H, W, esz))
        self.u0 = g.framed(nodes, fill, dt)
        self.ldp = We + ldp_extra
        self.ph0 = None
        if phase is not None:
            self.ph0 = np.full(He * self.ldp + 7, 0xEE, np.uint8)
            self.ph0[(np.arange(He)[:, None] * self.ldp + np.arange(We)[None, :]).ravel()] = phase.ravel()
        self.q0 = canary(B * 2 * He * ldq + 4 * vec, dt, byte) if fields else None
        self.part0 = canary(B * fx.NSUMS * per + PTAIL, np.float64, byte)
        self.sums0 = canary(B * fx.NSUMS + STAIL, np.float64, byte)
        up = lambda a: None if a is None else torch.from_numpy(a.view(np.uint8)).cuda()
        tu, tp, tq, tpart, tsums = (up(a) for a in (self.u0, self.ph0, self.q0, self.part0, self.sums0))
        ptr = lambda t: None if t is None else t.data_ptr()
        lib = _lib.lib()
        rc = getattr(lib, f"fea_flux_{suf}")(ptr(tu), ptr(tp), self.ldp, k[0], k[1], h, ptr(tq), ldq, He * ldq,
                                             2 * He * ldq, ptr(tpart), B, H, W, g.ld, g.bs, None)
        assert rc == 0, f"fea_flux_{suf} returned {rc}"
        rc = lib.fea_flux_final(ptr(tpart), per, ptr(tsums), B, None)
        assert rc == 0, f"fea_flux_final returned {rc}"
        torch.cuda.synchronize()
        down = lambda t, like: None if t is None else t.cpu().numpy().view(like.dtype)
        self.u1, self.ph1, self.q1 = down(tu, self.u0), down(tp, np.zeros(0, np.uint8)), down(tq, self.u0)
        self.part1, self.sums1 = down(tpart, self.part0), down(tsums, self.sums0)
        self.qmask = None
        if fields:
            self.qmask = np.zeros(self.q0.size, bool)
            self.qmask[:B * 2 * He * ldq].reshape(B, 2, He, ldq)[..., :We] = True

    @property
    def q(self):
        """[B, 2, He, We]"""
        B, He, We = self.B, self.H - 1, self.W - 1
        return self.q1[:B * 2 * He * self.ldq].reshape(B, 2, He, self.ldq)[..., :We]

    @property
    def part(self):
        return self.part1[:self.B * fx.NSUMS * self.per].reshape(self.B, fx.NSUMS, self.per)

    @property
    def sums(self):
        return self.sums1[:self.B * fx.NSUMS].reshape(self.B, fx.NSUMS)

    def check_footprint(self):
        """inputs unchanged; outside its write set every output still holds its canary; every element of a write set
        was stored"""
        assert _same(self.u0, self.u1).all(), "u modified"
        if self.ph0 is not None:
            assert np.array_equal(self.ph0, self.ph1), "phase modified"
        if self.q0 is not None:
            moved = ~_same(self.q0, self.q1)
            assert not (moved & ~self.qmask).any(), "q written outside the He x We elements (pad columns, tail)"
            assert (moved | ~self.qmask).all(), "q element never stored"
        n = self.B * fx.NSUMS * self.per
        assert _same(self.part0[n:], self.part1[n:]).all(), "part written beyond B * 5 * per"
        assert not _same(self.part0[:n], self.part1[:n]).any(), "a partial slot was never stored"
        n = self.B * fx.NSUMS
        assert _same(self.sums0[n:], self.sums1[n:]).all(), "sums written beyond B * 5"
        assert not _same(self.sums0[:n], self.sums1[:n]).any(), "a sum was never stored"


def bits(a):
    return np.ascontiguousarray(a).view(f"u{a.dtype.itemsize}")


def check_values(c, nodes, phase, suf, what):
    """q against the fp64 reference within the field bound and against numpy in T bit for bit; sums within theirs"""
    dt = NPDT[suf]
    ref = fx.element_values(nodes, phase, K0, K1, HSTEP, dt, wide=True)
    inT = fx.element_values(nodes, phase, K0, K1, HSTEP, dt)
    S = fx.companions(nodes, phase, K0, K1, HSTEP, dt)
    if c.q0 is not None:
        for j, name in enumerate(("q_r", "q_c")):
            err, bound = np.abs(c.q[:, j].astype(np.float64) - ref[name]), 2 * (N_TERMS + M_FACTORS) * U[suf] * S[name]
            print(f"{what} {name}: max err / bound = {(err / np.where(bound > 0, bound, 1)).max():.3g}")
            assert (err <= bound).all(), (what, name)
            assert np.array_equal(bits(c.q[:, j]), bits(inT[name])), (what, name, "not numpy's bits")
    want = fx.sums_of(inT)
    N = (c.H - 1) * (c.W - 1)
    for k, name in enumerate(fx.ORDER):
        Ssum = S[name].reshape(c.B, -1).sum(1)
        tol = U[suf] * np.abs(want[:, k]) + 2 * N * 2.0 ** -53 * Ssum
        err = np.abs(c.sums[:, k] - want[:, k])
        print(f"{what} sum {name}: max err / tol = {(err / tol).max():.3g}")
        assert (err <= tol).all(), (what, name, err, tol)


# ----------------------------------------------------------------------------- the kernel against flux_ref
@pytest.mark.parametrize("H, W", SHAPES)
@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_kernel_against_reference(suf, H, W):
    """Batches 1 and 3, with and without an image (pitched, non-zero bytes of any value count as 1), with and without
    the fields; a sample alone gives the bits it gives inside the batch; fields off gives the sums of fields on."""
    rng = np.random.default_rng([H, W, len(suf)])
    nodes = draw_u(rng, 3, H, W, suf)
    img = draw_phase(rng, H - 1, W - 1)
    for phase, extra in ((None, 0), (img, 0), (img, 5)):
        what = f"{suf} {H}x{W} {'no image' if phase is None else f'image pitch +{extra}'}"
        full = Call(suf, nodes, phase, True, ldp_extra=extra)
        full.check_footprint()
        check_values(full, nodes, phase, suf, what)
        only = Call(suf, nodes, phase, False, ldp_extra=extra)
        only.check_footprint()
        assert np.array_equal(bits(only.part), bits(full.part)) and np.array_equal(bits(only.sums), bits(full.sums))
        for b in range(3):
            one = Call(suf, nodes[b:b + 1], phase, True, ldp_extra=extra)
            one.check_footprint()
            assert np.array_equal(bits(one.q[0]), bits(full.q[b])), (what, b, "q differs from the batch's")
            assert np.array_equal(bits(one.part[0]), bits(full.part[b])), (what, b, "partials differ")
            assert np.array_equal(bits(one.sums[0]), bits(full.sums[b])), (what, b, "sums differ")
        if phase is None:   # k = k0 everywhere: the same as an all-zero image
            zero = Call(suf, nodes, np.zeros_like(img), True)
            assert np.array_equal(bits(zero.q), bits(full.q)) and np.array_equal(bits(zero.sums), bits(full.sums))


def test_host_layer_element_flux():
    """element_flux on plain tensors: the padded allocation's view, the means, prop rounded to float32."""
    from feanet_amd import element_flux
    rng = np.random.default_rng(5)
    for suf, (H, W) in (("f64", (9, 131)), ("f32", (7, 259)), ("f64", (5, 130))):
        nodes, img = draw_u(rng, 2, H, W, suf), draw_phase(rng, H - 1, W - 1)
        prop = (0.1, 20)
        k0, k1 = float(np.float32(0.1)), 20.0
        res = element_flux(torch.from_numpy(nodes).cuda().reshape(2, 1, H, W), torch.from_numpy(img != 0).cuda(),
                           prop=prop, h=HSTEP)
        assert res.q.shape == (2, 2, H - 1, W - 1) and res.q.dtype == TDT[suf] and res.q.is_cuda
        assert res.mean_flux.shape == (2, 2) and res.mean_grad.shape == (2, 2) and res.energy.shape == (2,)
        inT = fx.element_values(nodes, img, k0, k1, HSTEP, NPDT[suf])
        assert np.array_equal(bits(res.q[:, 0].cpu().numpy()), bits(inT["q_r"]))
        assert np.array_equal(bits(res.q[:, 1].cpu().numpy()), bits(inT["q_c"]))
        ref = Call(suf, nodes, img, True, k=(k0, k1))
        n = (H - 1) * (W - 1)
        assert np.array_equal(res.sums.cpu().numpy(), ref.sums)
        assert np.array_equal(res.mean_flux.cpu().numpy(), ref.sums[:, 0:2] / n)
        assert np.array_equal(res.mean_grad.cpu().numpy(), ref.sums[:, 2:4] / n)
        assert np.array_equal(res.energy.cpu().numpy(), ref.sums[:, 4])
        off = element_flux(torch.from_numpy(nodes).cuda(), torch.from_numpy(img).cuda() != 0, prop=prop, h=HSTEP,
                           fields=False)
        assert off.q is None and torch.equal(off.sums, res.sums)
    with pytest.raises(RuntimeError, match="MI355X"):
        element_flux(torch.zeros(1, 1, 5, 5))
    with pytest.raises(ValueError, match="phase image is"):
        element_flux(torch.zeros(1, 1, 5, 5, device="cuda"), np.zeros((5, 5), np.uint8))


# ----------------------------------------------------------------------------- task heights
LADDER_H, LADDER_W, RUNGS = 4097, 33, (1, 2, 4, 8, 16)


@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_batch_ladder_is_bitwise(suf):
    """H = 4097, W = 33 at batches 1, 2, 4, 8, 16: the framed kernels' task height runs through 2 .. 32 rows here;
    the flux kernel takes the height of ONE sample at every rung, so a sample's q, partials and sums are the same
    bits at every rung (the lower rungs are prefixes of the top rung's samples; the last sample also runs alone)."""
    from feanet_amd import _lib
    T, esz = TDT[suf], 4 if suf == "f32" else 8
    H, W, He, We = LADDER_H, LADDER_W, LADDER_H - 1, LADDER_W - 1
    ld, bs = _lib.mg_layout(H, W, esz)
    per = int(_lib.lib().fea_flux_parts(H, W, esz))
    assert per == fx.flux_parts(H, W, esz) == 2048
    gen = torch.Generator(device="cuda").manual_seed(7)
    top = RUNGS[-1]
    nodes = torch.randn((top, H, W), dtype=T, device="cuda", generator=gen)
    img = (torch.rand((He, We), device="cuda", generator=gen) < 0.4).to(torch.uint8)
    ldq = We

    def run(src):
        B = len(src)
        u = torch.zeros(B * bs + SLACK, dtype=T, device="cuda")
        torch.as_strided(u, (B, H, W), (bs, ld, 1), ld + 128 // esz - 1).copy_(nodes[list(src)])
        q = torch.empty((B, 2, He, ldq), dtype=T, device="cuda")
        part = torch.empty((B, fx.NSUMS, per), dtype=torch.float64, device="cuda")
        sums = torch.empty((B, fx.NSUMS), dtype=torch.float64, device="cuda")
        lib = _lib.lib()
        assert getattr(lib, f"fea_flux_{suf}")(u.data_ptr(), img.data_ptr(), We, K0, K1, HSTEP, q.data_ptr(), ldq,
                                               He * ldq, 2 * He * ldq, part.data_ptr(), B, H, W, ld, bs, None) == 0
        assert lib.fea_flux_final(part.data_ptr(), per, sums.data_ptr(), B, None) == 0
        torch.cuda.synchronize()
        return q, part, sums

    def same(a, b):
        v = {4: torch.int32, 8: torch.int64}[a.element_size()]
        return torch.equal(a.contiguous().view(v), b.contiguous().view(v))
    tq, tpart, tsums = run(range(top))
    assert bool(torch.isfinite(tsums).all())
    for src in [tuple(range(k)) for k in RUNGS[:-1]] + [(top - 1,)]:
        q, part, sums = run(src)
        for i, b in enumerate(src):
            assert same(q[i], tq[b]) and same(part[i], tpart[b]) and same(sums[i], tsums[b]), (len(src), b)
    # the top rung's first sample against the reference (the tall grid: every row task but the last is 2 rows high)
    n0 = nodes[:1].cpu().numpy()
    inT = fx.element_values(n0, img.cpu().numpy(), K0, K1, HSTEP, NPDT[suf])
    assert np.array_equal(bits(tq[0, 0].cpu().numpy()), bits(inT["q_r"][0]))
    assert np.array_equal(bits(tq[0, 1].cpu().numpy()), bits(inT["q_c"][0]))


# ----------------------------------------------------------------------------- nontemporal stores
def child_main(out):
    """(child process) one call with the fields on fixed data; FEANET_NT_BYTES comes from the environment"""
    rng = np.random.default_rng(11)
    res = {}
    for suf, (H, W) in (("f32", (34, 258)), ("f64", (9, 131))):
        nodes, img = draw_u(rng, 2, H, W, suf), draw_phase(rng, H - 1, W - 1)
        c = Call(suf, nodes, img, True)
        c.check_footprint()
        res[f"q_{suf}"], res[f"part_{suf}"], res[f"sums_{suf}"] = c.q1, c.part1, c.sums1
    np.savez(out, **res)


def test_nontemporal_stores_give_the_same_bits(tmp_path):
    """FEANET_NT_BYTES=0 (every q streams past the caches) against a threshold no field reaches, each in a fresh
    process: the same bytes in q (pad columns' canaries included), the partials and the sums."""
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


# ----------------------------------------------------------------------------- footprint
@pytest.mark.parametrize("suf", ["f32", "f64"])
def test_footprint_and_padding_independence(suf):
    """Run Z (zeros in the ghost ring, the pad columns and the slack between and behind the samples, canary C1 in the
    outputs) against run P (quiet NaNs there, canary C2): the same bits on every write set, canaries untouched
    around them, inputs unchanged.  Then one NaN node: exactly its own sample's five sums are non-finite."""
    for H, W in ((3, 3), (9, 131), (34, 258), (7, 259)):
        rng = np.random.default_rng([H, W, 3])
        nodes, img = draw_u(rng, 3, H, W, suf), draw_phase(rng, H - 1, W - 1)
        z = Call(suf, nodes, img, True, fill=0.0, byte=C1, ldp_extra=3)
        p = Call(suf, nodes, img, True, fill=np.nan, byte=C2, ldp_extra=3)
        assert np.isnan(p.u0[~p.geo.nodes()]).all() and not np.isnan(p.u0[p.geo.nodes()]).any()
        z.check_footprint(), p.check_footprint()
        assert np.array_equal(bits(z.q), bits(p.q)), (H, W, "q depends on non-node storage")
        assert np.array_equal(bits(z.part), bits(p.part)) and np.array_equal(bits(z.sums), bits(p.sums)), (H, W)
        assert np.isfinite(z.sums).all()
        for j, (r, c) in ((0, (0, 0)), (1, (H // 2, W - 2)), (2, (H - 1, W - 1))):
            bad = nodes.copy()
            bad[j, r, c] = np.nan
            n = Call(suf, bad, img, True, fill=np.nan)
            for b in range(3):
                if b == j:
                    assert not np.isfinite(n.sums[b]).any(), (H, W, j, "a NaN node left a sum finite")
                else:
                    assert np.array_equal(bits(n.sums[b]), bits(z.sums[b])), (H, W, j, b, "leak between samples")
                    assert np.array_equal(bits(n.q[b]), bits(z.q[b])), (H, W, j, b)


# ----------------------------------------------------------------------------- the solvers
RTOL = 1e-10
SIZES = [(64, 64), (48, 96)]


def residual_bound(name, m, n, prop):
    """How far K_eff can be off when every load case stops at ||r|| <= rtol ||r0||, in units of rtol max|K_eff|.
    With x_i the linear field, u_i the exact discrete solution, d_i = u_i - x_i (zero on the boundary) and dv the
    error of an iterate (zero on the boundary too): sum q_i(v) = -a(v, x_i) for any v, since grad x_i = e_i; and
    a(dv_j, u_i) = 0 because K u_i vanishes on the interior rows and dv_j on the others.  So
        |V| dK_eff[i, j] = a(dv_j, x_i) = -a(dv_j, d_i) = d_i . r_j       (r_j = -K dv_j, the residual)
        |dK_eff[i, j]| <= ||d_i|| ||r_j|| / |V| <= rtol ||d_i|| ||r0_j|| / |V|,        r0_j = -(K x_j) on the interior.
    Evaluated on the dense reference; test_effective_conductivity asserts that it stays below the 100 the test allows
    (it is 6.3 at most on these images), so 100 rtol leaves room for the float32 table's asymmetry and the sums'
    and the dense solve's roundoff, all far below rtol = 1e-10 times these factors."""
    ref = fx.homogenize_image(name, m, n, prop)
    K = fx.assemble_table(pr.image(name, m, n), prop)
    x = fx.load_cases(m, n, 2.0).reshape(2, -1)
    inner = np.zeros((m + 1, n + 1), bool)
    inner[1:-1, 1:-1] = True
    r0 = (K @ x.T).T[:, inner.ravel()]
    d = ref["u"].reshape(2, -1) - x
    V = m * n * (2.0 / n) ** 2
    return max(np.linalg.norm(d[i]) * np.linalg.norm(r0[j]) for i in range(2) for j in range(2)) / V / \
        np.abs(ref["K_eff"]).max()


@pytest.mark.parametrize("mixed", [False, True], ids=["fp64", "mixed"])
@pytest.mark.parametrize("prop", [(1, 20), (20, 1)])
@pytest.mark.parametrize("name", ["six_discs", "stripes"])
@pytest.mark.parametrize("m, n", SIZES)
def test_effective_conductivity(m, n, name, prop, mixed):
    """PCG (fp64, and fp64 around an fp32 cycle) against the dense pipeline on the same float32 table: within
    100 rtol of max|K_eff| (residual_bound), every sample converged, Hill's identity within the host test's bound."""
    from feanet_amd import effective_conductivity
    ref = fx.homogenize_image(name, m, n, prop)
    factor = residual_bound(name, m, n, prop)
    assert factor <= 100.0 / 4, f"the stopping rule allows {factor:.1f} rtol max|K_eff| here: 100 rtol is not justified"
    kw = dict(precond_dtype=torch.float32) if mixed else {}
    res = effective_conductivity(pr.image(name, m, n), prop=prop, rtol=RTOL, **kw)
    assert res.flags.tolist() == [1, 1] and res.converged, f"flags {res.flags}, iterations {res.iterations}"
    scale = np.abs(ref["K_eff"]).max()
    err = np.abs(res.K_eff - ref["K_eff"]).max() / scale
    print(f"{m}x{n} {name} {prop}: iterations {res.iterations.tolist()}, K_eff error {err:.2e} of max|K_eff| "
          f"(allowed {100 * RTOL:.0e}, stopping-rule factor {factor:.1f}), Hill {res.hill_defect.max():.2e}")
    assert res.K_eff.shape == (2, 2) and res.K_eff.dtype == np.float64
    assert err <= 100 * RTOL
    assert np.abs(res.energy - ref["energy"]).max() <= 100 * RTOL * ref["energy"].max()
    assert np.abs(res.mean_grad - np.eye(2)).max() <= 1e-10
    assert res.hill_defect.max() <= HILL_BOUND
    if name == "stripes":   # vertical stripes: along r the arithmetic mean (the dense pipeline holds it to 1e-9)
        assert abs(res.K_eff[0, 0] - 10.5) <= 1e-9 + 100 * RTOL * 10.5


@pytest.mark.parametrize("method", ["pcg", "mg"])
@pytest.mark.parametrize("value", [0, 1])
@pytest.mark.parametrize("m, n", SIZES)
def test_homogeneous_image(m, n, value, method):
    """Both samples converged and K_eff = k I within the field bound of the element fluxes (the linear load cases; S
    as in the module docstring; the sums of g telescope to the boundary data, so this holds for any field with it).
    Where h is a power of two (n = 64) every r h is exact, K annihilates the linear field exactly (the table's rows
    are one float32 number times (-2 .. 16 .. -2)), so r0 = 0: no iteration, exactly 0 off the diagonal.  At n = 96,
    h = 1/48: fl((r-1) h) + fl((r+1) h) != 2 fl(r h), r0 is rounding noise and not 0, and the iteration count is
    not pinned."""
    from feanet_amd import effective_conductivity
    prop = (1, 20)
    res = effective_conductivity(np.full((m, n), value, np.uint8), prop=prop, method=method)
    print(f"{m}x{n} value {value} {method}: iterations {res.iterations.tolist()}, flags {res.flags.tolist()}")
    assert res.flags.tolist() == [1, 1]
    k = float(prop[value])
    S = fx.companions(fx.load_cases(m, n, 2.0), None, k, k, 2.0 / n, np.float64)["q_r"].reshape(2, -1).mean(1)
    tol = 2 * (N_TERMS + M_FACTORS) * 2.0 ** -53 * S.max()
    assert np.abs(res.K_eff - k * np.eye(2)).max() <= tol
    if n & (n - 1) == 0:
        assert res.iterations.tolist() == [0, 0]
        assert res.K_eff[0, 1] == 0 and res.K_eff[1, 0] == 0 and np.array_equal(res.K_eff, k * np.eye(2))


def test_multigrid_method_and_refusals():
    from feanet_amd import effective_conductivity
    # (stripes: the stationary cycle contracts by about 0.77 per cycle with coarsen="stiff"; on the six
    # discs it needs more than 200 cycles for 1e-10)
    ref = fx.homogenize_image("stripes", 64, 64, (1, 20))
    res = effective_conductivity(pr.stripes(64, 64), prop=(1, 20), method="mg", rtol=RTOL, max_iters=200)
    assert res.flags.tolist() == [1, 1], f"flags {res.flags}, cycles {res.iterations}"
    assert np.abs(res.K_eff - ref["K_eff"]).max() <= 100 * RTOL * np.abs(ref["K_eff"]).max()
    # max_iters too small: reported, not hidden, and no exception
    short = effective_conductivity(pr.six_discs(64, 64), prop=(1, 20), rtol=RTOL, max_iters=2)
    assert short.flags.tolist() == [0, 0] and not short.converged and short.iterations.tolist() == [2, 2]


@pytest.mark.parametrize("T", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("problem", ["interface", "poisson"])
def test_multigrid_solver_flux_reads_the_current_iterate(problem, T):
    """MultigridSolver(shape=0) and the Poisson problem after joined cycles (the iterate rests mid-cycle): flux() is
    the kernel on the field solution() returns, with element_phase(N, 0, size) as the image, k = 1 for Poisson."""
    from feanet_amd import MultigridSolver, mesh_setup as ms
    suf = "f32" if T == torch.float32 else "f64"
    n, B = 64, 2
    rng = np.random.default_rng(9)
    s = MultigridSolver(n, problem=problem, dtype=T, batch=B, prop=(1, 20), shape=0)
    s.set_boundary(torch.from_numpy(rng.standard_normal((B, 1, n + 1, n + 1))).cuda().to(T))
    s.set_rhs(f=torch.from_numpy(rng.standard_normal((B, 1, n + 1, n + 1))).cuda().to(T))
    s.load()
    s.vcycle(3)
    res = s.flux()
    u = s.solution().cpu().numpy()[:, 0]
    img = ms.element_phase(n + 1, 0, 2.0).astype(np.uint8) if problem == "interface" else None
    k1 = 20.0 if problem == "interface" else 1.0
    inT = fx.element_values(u, img, 1.0, k1, 2.0 / n, NPDT[suf])
    assert np.array_equal(bits(res.q[:, 0].cpu().numpy()), bits(inT["q_r"]))
    assert np.array_equal(bits(res.q[:, 1].cpu().numpy()), bits(inT["q_c"]))
    want = fx.sums_of(inT)
    S = fx.companions(u, img, 1.0, k1, 2.0 / n, NPDT[suf])
    got = res.sums.cpu().numpy()
    for k, name in enumerate(fx.ORDER):
        tol = U[suf] * np.abs(want[:, k]) + 2 * n * n * 2.0 ** -53 * S[name].reshape(B, -1).sum(1)
        assert (np.abs(got[:, k] - want[:, k]) <= tol).all(), name
    off = s.flux(fields=False)
    assert off.q is None and torch.equal(off.sums, res.sums)


def test_pcg_solver_flux_mixed_reads_the_fp64_iterate():
    from feanet_amd import PCGSolver
    m, n = 48, 96
    img = pr.six_discs(m, n)
    s = PCGSolver(n, rows=m, problem="interface", batch=2, prop=(1, 20), phase=img, coarsen="stiff",
                  precond_dtype=torch.float32)
    u0 = torch.from_numpy(fx.load_cases(m, n, 2.0)).cuda().reshape(2, 1, m + 1, n + 1)
    bc = u0.clone()
    bc[..., 1:-1, 1:-1] = 0
    s.solve(u0=u0, f=torch.zeros_like(u0), rtol=1e-6, max_iters=50, bc_value=bc)
    res = s.flux()
    assert res.q.dtype == torch.float64
    inT = fx.element_values(s.solution().cpu().numpy()[:, 0], img, 1.0, 20.0, 2.0 / n, np.float64)
    assert np.array_equal(bits(res.q[:, 0].cpu().numpy()), bits(inT["q_r"]))
    assert np.array_equal(bits(res.q[:, 1].cpu().numpy()), bits(inT["q_c"]))


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child_main(sys.argv[2])
