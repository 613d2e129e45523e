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

FluxResult = namedtuple("FluxResult", "q mean_flux mean_grad energy sums")
FluxResult.__doc__ = """q: [B, 2, He, We] element fluxes (q_r, q_c) in the field's dtype, or None (fields=False); a
view of a padded allocation where We is not a multiple of 16 / itemsize.  mean_flux, mean_grad: [B, 2] float64, the
element means (sum / (He We)).  energy: [B] float64, sum over the elements of k u_e^T Ke u_e (= u^T K u).  sums: the raw
[B, 5] sums."""


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
    ops.require_hip(u, "u")
    if u.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"feanet_amd.flux: u must be float32 or float64, got {u.dtype}")
    if u.dim() < 2:
        raise ValueError("feanet_amd.flux: u must be [B, 1, H, W]")
    H, W = u.shape[-2:]
    B = u.numel() // (H * W) if H * W else 0
    if B < 1:
        raise ValueError("feanet_amd.flux: u is empty")
    u = u.reshape(B, 1, H, W).contiguous()
    esz = u.element_size()
    ld, bs = _lib.mg_layout(H, W, esz)
    img = phase_operand(phase, H - 1, W - 1, u.device)
    k0, k1 = coefficients(prop)
    framed = torch.zeros(B * bs + 256, dtype=u.dtype, device=u.device)
    _lib.call("mg_pack", u.dtype, u.data_ptr(), framed.data_ptr(), None, -1, None, 0, B, H, W, ld, bs, ops._stream(u))
    return flux_framed(framed.data_ptr(), u.dtype, u.device, B, H, W, ld, bs, img, k0, k1, h, fields)
