"""Element flux fields q = -k grad u, their means, the mean gradient and the stored energy of a nodal field
(include/feanet_flux.h, csrc/flux_ops.hip; definitions: DESIGN §16).

Grid axes: component 0 is along the row index r (coordinate r h), component 1 along the column index c.  Everything
stays on the device and nothing synchronises: FluxResult holds device tensors.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib, mesh_setup as ms, ops

NSUMS = 5  # FEA_FLUX_NSUMS: q_r, q_c, g_r, g_c, e
ENERGY_NSUMS = 6  # FEA_ENERGY_NSUMS: uu, uv, vv, each over phase 0 then phase 1

FluxResult = namedtuple("FluxResult", "q mean_flux mean_grad energy sums")
FluxResult.__doc__ = """q: [B, 2, He, We] element fluxes (q_r, q_c) in the field's dtype, or None (fields=False); a
view of a padded allocation where We is not a multiple of 16 / itemsize.  mean_flux, mean_grad: [B, 2] float64, the
element means (sum / (He We)).  energy: [B] float64, sum over the elements of k u_e^T Ke u_e (= u^T K u).  sums: the raw
[B, 5] sums."""


EnergyForms = namedtuple("EnergyForms", "A density")
EnergyForms.__doc__ = """A: [B, 2 phases, 3] float64, A[b, p] = (sum over the elements of phase p of d(u,u), d(u,v),
d(v,v)) of pair b, d(u, v) = u_e^T Ke v_e (include/feanet_energy.h): the energy form is a(u, v) = k0 A[:, 0, 1] +
k1 A[:, 1, 1].  density: [B, 3, He, We] in the field's dtype, the three d per element (uu, uv, vv), or None
(fields=False); a view of a padded allocation where We is not a multiple of 16 / itemsize."""


def coefficients(prop):
    """(k0, k1) as the solver's stencil table has them: rounded to float32."""
    return float(np.float32(prop[0])), float(np.float32(prop[1]))


def phase_operand(phase, He, We, device):
    """A phase image as the kernel reads it: a contiguous uint8 [He, We] device tensor (None stays None)."""
    if phase is None:
        return None
    img = ms._phase_tensor(phase, device)
    if tuple(img.shape) != (He, We):
        raise ValueError(f"feanet_amd.flux: the phase image is {tuple(img.shape)}, the field has {He} x {We} elements")
    return img


def flux_framed(ptr, dtype, device, B, H, W, ld, bstride, phase=None, k0=1.0, k1=1.0, h=1.0, fields=True):
    """fea_flux + fea_flux_final on a level-0 framed buffer at device address `ptr`; phase: None or a contiguous uint8
    [H-1, W-1] device tensor."""
    esz = 4 if dtype == torch.float32 else 8
    He, We = H - 1, W - 1
    per = int(_lib.lib().fea_flux_parts(H, W, esz))
    if per < 1:
        raise ValueError(f"feanet_amd.flux: unsupported grid {H} x {W}")
    part = torch.empty(B * NSUMS * per, dtype=torch.float64, device=device)
    sums = torch.empty((B, NSUMS), dtype=torch.float64, device=device)
    q, qp, ldq = None, None, 0
    if fields:
        vec = 16 // esz
        ldq = -(-We // vec) * vec
        q = torch.empty((B, 2, He, ldq), dtype=dtype, device=device)
        qp = q.data_ptr()
    stream = torch.cuda.current_stream(device).cuda_stream
    _lib.call("flux", dtype, ptr, None if phase is None else phase.data_ptr(), We, float(k0), float(k1), float(h), qp,
              ldq, He * ldq, 2 * He * ldq, part.data_ptr(), B, H, W, ld, bstride, stream)
    _lib.call_raw("flux_final", part.data_ptr(), per, sums.data_ptr(), B, stream)
    n = torch.full((), float(He * We), dtype=torch.float64, device=device)  # a tensor divisor: a true division
    return FluxResult(None if q is None else q[..., :We], sums[:, 0:2] / n, sums[:, 2:4] / n, sums[:, 4].clone(), sums)


def element_flux(u, phase=None, prop=(1, 1), h=1.0, fields=True):
    """Flux fields and sums of any [B, 1, H, W] (or [B, H, W] / [H, W]) float32 / float64 device tensor: element
    (R, C) has the nodes u[R:R+2, C:C+2] and the coefficient prop[phase[R, C]] (phase None: prop[0]); h is the node
    spacing.  The field is copied into a framed scratch buffer first (fea_mg_pack, a raw copy)."""
    framed, B, H, W, ld, bs = _framed_copy(u, "u")
    img = phase_operand(phase, H - 1, W - 1, u.device)
    k0, k1 = coefficients(prop)
    return flux_framed(framed.data_ptr(), u.dtype, u.device, B, H, W, ld, bs, img, k0, k1, h, fields)


def energy_framed(uptr, vptr, dtype, device, B, H, W, ld, ubstride, vbstride, phase=None, fields=True):
    """fea_energy + fea_energy_final on level-0 framed buffers at the device addresses `uptr`, `vptr` (pair b: uptr +
    b * ubstride elements with vptr + b * vbstride); phase: None or a contiguous uint8 [H-1, W-1] device tensor."""
    esz = 4 if dtype == torch.float32 else 8
    He, We = H - 1, W - 1
    per = int(_lib.lib().fea_energy_parts(H, W, esz))
    if per < 1:
        raise ValueError(f"feanet_amd.flux: unsupported grid {H} x {W}")
    part = torch.empty(B * ENERGY_NSUMS * per, dtype=torch.float64, device=device)
    sums = torch.empty((B, 3, 2), dtype=torch.float64, device=device)
    dens, dp, ldd = None, None, 0
    if fields:
        vec = 16 // esz
        ldd = -(-We // vec) * vec
        dens = torch.empty((B, 3, He, ldd), dtype=dtype, device=device)
        dp = dens.data_ptr()
    stream = torch.cuda.current_stream(device).cuda_stream
    _lib.call("energy", dtype, uptr, vptr, None if phase is None else phase.data_ptr(), We, dp, ldd, He * ldd,
              3 * He * ldd, part.data_ptr(), B, H, W, ld, ubstride, vbstride, stream)
    _lib.call_raw("energy_final", part.data_ptr(), per, sums.data_ptr(), B, stream)
    return EnergyForms(sums.transpose(1, 2), None if dens is None else dens[..., :We])


def _framed_copy(u, what):
    """(framed copy, B, H, W, ld, bstride) of any [B, 1, H, W] (or [B, H, W] / [H, W]) float device tensor"""
    ops.require_hip(u, what)
    if u.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"feanet_amd.flux: {what} must be float32 or float64, got {u.dtype}")
    if u.dim() < 2:
        raise ValueError(f"feanet_amd.flux: {what} must be [B, 1, H, W]")
    H, W = u.shape[-2:]
    B = u.numel() // (H * W) if H * W else 0
    if B < 1:
        raise ValueError(f"feanet_amd.flux: {what} is empty")
    u = u.reshape(B, 1, H, W).contiguous()
    ld, bs = _lib.mg_layout(H, W, u.element_size())
    framed = torch.zeros(B * bs + 256, dtype=u.dtype, device=u.device)
    _lib.call("mg_pack", u.dtype, u.data_ptr(), framed.data_ptr(), None, -1, None, 0, B, H, W, ld, bs, ops._stream(u))
    return framed, B, H, W, ld, bs


def energy_forms(u, v=None, phase=None, fields=True):
    """The energy forms d(u,u), d(u,v), d(v,v) of two [B, 1, H, W] (or [B, H, W] / [H, W]) float32 / float64 device
    tensors of one shape and dtype, summed per phase of the element image `phase` (None: every element is phase 0),
    and their element densities, as an EnergyForms of device tensors.  v None: v = u.  Each field is copied into a
    framed scratch buffer first (fea_mg_pack, a raw copy); nothing synchronises."""
    fu, B, H, W, ld, bs = _framed_copy(u, "u")
    fv = fu
    if v is not None:
        if not torch.is_tensor(v) or v.dtype != u.dtype or v.device != u.device:
            raise TypeError("feanet_amd.flux: v must be a tensor of u's dtype on u's device")
        if v.dim() < 2 or tuple(v.shape[-2:]) != (H, W) or v.numel() != B * H * W:
            raise ValueError(f"feanet_amd.flux: v has shape {tuple(v.shape)}, u has {tuple(u.shape)}")
        fv = _framed_copy(v, "v")[0]
    img = phase_operand(phase, H - 1, W - 1, u.device)
    return energy_framed(fu.data_ptr(), fv.data_ptr(), u.dtype, u.device, B, H, W, ld, bs, bs, img, fields)


def pair_forms(ptr, dtype, device, batch, geom, pair, phase, fields, who):
    """energy_framed on samples pair[0], pair[1] of a solver's resident framed iterate at `ptr` (geom: B, H, W, ld,
    bstride)"""
    _, H, W, ld, bs = geom
    i, j = (int(p) for p in pair)
    if not (0 <= i < batch and 0 <= j < batch):
        raise ValueError(f"{who}: pair {tuple(pair)} is outside a batch of {batch}")
    esz = 4 if dtype == torch.float32 else 8
    return energy_framed(ptr + i * bs * esz, ptr + j * bs * esz, dtype, device, 1, H, W, ld, bs, bs, phase, fields)
