"""ctypes binding of libfeanet_hip.so (C ABI: include/feanet_hip.h).

The product path has no CPU fallback: if the library is missing or no HIP device is present,
every op raises.  `torch` is imported first so the library binds to the HIP runtime torch
loaded (libamdhip64.so.7), not a second copy.
"""
import ctypes
import os

import torch  # noqa: F401  (must precede the CDLL load)

from .build import LIB

_IN_TREE = LIB

ABI_VERSION = 3

P = ctypes.c_void_p
I = ctypes.c_int
LL = ctypes.c_longlong
F32 = ctypes.c_float
F64 = ctypes.c_double

# name -> "TYPE param, ..." as declared in include/feanet_hip.h, in that order (tests/test_abi.py compares the two).
# TYPE: P pointer, I int, LL long long, S the scalar T of the _f32/_f64 pair (which shares the signature otherwise),
# D double, PI / PLL int* / long long* results.  `stream` is last everywhere and is not part of a launch record.
_CTYPES = {"P": P, "I": I, "LL": LL, "S": "S", "D": F64, "PI": ctypes.POINTER(I), "PLL": ctypes.POINTER(LL)}
_SIGS = {
    "knet_apply": "P u, P y, P pid, P ktab, I ntab, I B, I H, I W, P stream",
    "split_x": "P x, P xs, P pid, I C, I B, I H, I W, P stream",
    "jacobi_sweep": "P u, P f, P out, P pid, P ktab, P omd, I ntab, P geo, LL geo_bstride, P bc, LL bc_bstride, "
                    "I B, I H, I W, P stream",
    "residual": "P u, P f, P r, P pid, P ktab, I ntab, I B, I H, I W, P stream",
    "jacobi_sweep_pbc": "P u, P f, P out, P ktab, P omd, I B, I N, P stream",
    "pbc_pad": "P u, P dst, I B, I N, I lo, I hi, P stream",
    "restrict": "P x, I C, P fc, P pid, P rtab, I ntab, S w0, I B, I H, I W, P stream",
    "prolong": "P e, I C, P out, P add, P pidc, P ptab, I ntab, S w1, I B, I Hc, I Wc, P stream",
    "residual_norm": "P u, P f, P pid, P ktab, I ntab, P out, P ws, I B, I H, I W, P stream",
    # adjoints (autograd)
    "knet_apply_adj": "P g, P out, P pid, P ktab, I ntab, I B, I H, I W, P stream",
    "jacobi_sweep_adj": "P g, P gu, P gf, P pid, P ktab, P omd, I ntab, P geo, LL geo_bs, I B, I H, I W, P stream",
    "restrict_adj": "P g, I C, P gx, P pid, P rtab, I ntab, S w0, I B, I H, I W, P stream",
    "prolong_adj": "P g, I C, P ge, P pidc, P ptab, I ntab, S w1, I B, I Hc, I Wc, P stream",
    "transfer_weight_grad": "P cf, I c_split, P ff, I f_split, I C, I interior, S scale, P gw, P ws, I B, I Hc, "
                            "I Wc, P stream",
    "stencil_weight_grad": "P g, P u, P pid, I ntab, S scale, P gw, P ws, I B, I H, I W, P stream",
    # framed level ops
    "mg_pack": "P src, P dst, P geo, LL geo_bstride, P bc, LL bc_bstride, I B, I H, I W, I ld, LL bstride, P stream",
    "mg_unpack": "P src, P dst, I B, I H, I W, I ld, LL bstride, P stream",
    "mg_sweep": "P u, P f, P out, P pid, P ktab, P omd, I ntab, I B, I H, I W, I ld, LL bstride, P stream",
    "mg_residual_restrict": "P u, P f, P v_out, P fc, P pid, P ktab, P omd, I ntab, P rtab, I nrtab, S w0, I B, "
                            "I H, I W, I ld, LL bstride, I ldc, LL bstridec, P stream",
    "mg_zero_restrict2": "P f, P fc, P fc2, P pid, P pidc, P ktab, P omd, I ntab, P rtab, I nrtab, S w0, I B, I H, "
                         "I W, I ld, LL bstride, I ldc, LL bstridec, I ldc2, LL bstridec2, P stream",
    "mg_zero_restrict2_send": "P f, P fc, P fc2, P pid, P pidc, P ktab, P omd, I ntab, P rtab, I nrtab, S w0, I B, "
                              "I H, I W, I ld, LL bstride, I ldc, LL bstridec, I ldc2, LL bstridec2, P send, I r0, "
                              "I r1, I c0, I c1, P stream",
    "mg_zero_restrict_send": "P f, P fc, P pid, P ktab, P omd, I ntab, P rtab, I nrtab, S w0, I B, I H, I W, I ld, "
                             "LL bstride, I ldc, LL bstridec, P send, I r0, I r1, I c0, I c1, P stream",
    "mg_sweep_restrict": "P u, P f, P u_out, P fc, P pid, P ktab, P omd, I ntab, P rtab, I nrtab, S w0, I B, I H, "
                         "I W, I ld, LL bstride, I ldc, LL bstridec, P norm_ws, P norm_hist, P norm_cnt, P stream",
    "mg_prolong_sweep": "P u, P ec, P f, P out, P pid, P pidc, P ktab, P omd, I ntab, P ptab, I nptab, S w1, I B, "
                        "I H, I W, I ld, LL bstride, I ldc, LL bstridec, P stream",
    "mg_prolong2": "P fc, P ec2, P f, P out, P pid, P pidc, P pidc2, P ktab, P omd, I ntab, P ptab, I nptab, S w1, "
                   "I B, I H, I W, I ld, LL bstride, I ldc, LL bstridec, I ldc2, LL bstridec2, P stream",
    "mg_prolong_add": "P u, P ec, P out, P pidc, P ptab, I nptab, S w1, I B, I H, I W, I ld, LL bstride, I ldc, "
                      "LL bstridec, P stream",
    "mg_residual_norm": "P u, P f, P pid, P ktab, I ntab, P out, P ws, I B, I H, I W, I ld, LL bstride, I rlo, "
                        "I rhi, I clo, I chi, P stream",
    "mg_cycle_join": "P u, P ec, P f, P u_out, P fc, P pid, P pidc, P ktab, P omd, I ntab, P ptab, I nptab, P rtab, "
                     "I nrtab, S w1, S w0, I B, I H, I W, I ld, LL bstride, I ldc, LL bstridec, P norm_ws, "
                     "P norm_hist, P norm_cnt, P stream",
    "mg_cycle_join_rects": "P u, P ec, P f, P u_out, P fc, P pid, P pidc, P ktab, P omd, I ntab, P ptab, I nptab, "
                           "P rtab, I nrtab, S w1, S w0, I B, I H, I W, I ld, LL bstride, I ldc, LL bstridec, "
                           "I nrect, P rects, P stream",
    "mg_hsweep": "P u, P u_raw, P f, P out, P pid, P ktab, P omd, I ntab, P hw, I nlayers, I B, I H, I W, I ld, "
                 "LL bstride, P stream",
    "mg_hsweep_restrict": "P u, P u_raw, P f, P out, P fc, P pid, P ktab, P omd, I ntab, P hw, I nlayers, P rtab, "
                          "I nrtab, S w0, I B, I H, I W, I ld, LL bstride, I ldc, LL bstridec, P stream",
    "mg_prolong_hsweep": "P u, P u_raw, P ec, P f, P out, P pid, P pidc, P ktab, P omd, I ntab, P hw, I nlayers, "
                         "P ptab, I nptab, S w1, I B, I H, I W, I ld, LL bstride, I ldc, LL bstridec, P stream",
    "mg_coarse_tail": "P f_t, P v_t, I Ht, I Wt, I nlev, I ld_t, LL bs_t, P pid_levels, P ktab, P omd, I ntab, "
                      "P rtab, P ptab, S w0, S w1, I nu1, I nu2, I q2, I B, P stream",
    "mg_coarse_tail_ext": "P f_x, P v_x, I Hx, I Wx, I ld_x, LL bs_x, I nlev, P ktab, P omd, I ntab, P rtab, "
                          "P ptab, S w0, S w1, I B, P stream",
    "mg_hjac_tail": "P f_t, P u_t, I Ht, I Wt, I nlev, I ld_t, LL bs_t, P pid_levels, P ktab, P omd, I ntab, "
                    "P rtab, P ptab, P hw, I nlayers, S w0, S w1, I nu1, I nu2, I B, P stream",
    # several coarse levels per launch (pointer arrays: PtrArray)
    "mg_mid_down": "P f, P pid, I k, I B, I H, I W, P ktab, P omd, I ntab, P rtab, I nrtab, S w0, I TR, I TC, P stream",
    "mg_mid_down_gathered": "P f, P pid, I k, I B, I H, I W, P ktab, P omd, I ntab, P rtab, I nrtab, S w0, I TR, "
                            "I TC, P gsrc, I Pr, I Pc, I gcr, I gcc, P stream",
    "mg_mid_up": "P f, P e, P out, P pid, I k, I B, I H, I W, P ktab, P omd, I ntab, P ptab, I nptab, S w1, I TR, "
                 "I TC, P stream",
    "mg_hmid_down": "P f, P u, P pid, I B, I H, I W, P ktab, P omd, I ntab, P hw, I nlayers, P rtab, I nrtab, S w0, "
                    "I T, P stream",
    "mg_hmid_up": "P f, P u, P e, P out, P pid, I B, I H, I W, P ktab, P omd, I ntab, P hw, I nlayers, P ptab, "
                  "I nptab, S w1, I T, P stream",
    # Krylov vector operations (feanet_amd.pcg)
    "pcg_residual": "P x, P f, P r, P pid, P ktab, I ntab, P part, I B, I H, I W, I ld, LL bstride, P stream",
    "pcg_direction": "P z, P p_in, P p_out, P pid, P ktab, I ntab, P scalars, P part, I B, I H, I W, I ld, "
                     "LL bstride, P stream",
    "pcg_update": "P p, P x, P r, P pid, P ktab, I ntab, P scalars, P part, I B, I H, I W, I ld, LL bstride, P stream",
    "pcg_dot": "P r, P z, P part, I B, I H, I W, I ld, LL bstride, P stream",
}
_EXTRA = {
    "fea_abi_version": ("", I),
    "fea_mg_layout": ("I H, I W, I elem_size, PI ld, PLL bstride", I),
    "fea_norm_workspace_bytes": ("I B, I H, I W", ctypes.c_size_t),
    "fea_mg_join_norm_parts": ("I B, I H, I W, I elem_size", LL),
    "fea_norm_append": ("P ws, LL stride, LL per, I B, I nrows, P hist, P cnt, P stream", I),
    "fea_mg_coarse_tail_lds_bytes": ("I Ht, I Wt, I nlev, I elem_size, I multi", ctypes.c_size_t),
    "fea_mg_hjac_tail_lds_bytes": ("I Ht, I Wt, I nlev, I elem_size, I multi", ctypes.c_size_t),
    "fea_mg_mid_lds_bytes": ("I up, I k, I TR, I TC, I elem_size, I multi", LL),
    "fea_mg_hmid_lds_bytes": ("I up, I T, I nlayers, I elem_size, I multi", LL),
    "fea_interface_pattern_map": ("P out, LL ld, I N, I shape, D size, P stream", I),
    "fea_dd_copy_blocks": ("P blocks, I nblocks, I elem_size, I to_stage, P stream", I),
    "fea_dd_copy_rects": ("P rects, I nrects, I elem_size, P stream", I),
    "fea_pcg_parts": ("I H, I W, I elem_size", LL),
    "fea_pcg_scalar_step": ("P part, LL per, P scalars, P hist, I hist_rows, I B, I step, P stream", I),
    # fp64 Krylov fields with an fp32 preconditioner
    "fea_pcg_narrow_f64f32": ("P r, P r32, P scalars, P sb, I B, I H, I W, I ld, LL bstride, I ld32, LL bstride32, "
                              "P stream", I),
    "fea_pcg_dot_f64f32": ("P r, P z32, P part, I B, I H, I W, I ld, LL bstride, I ld32, LL bstride32, P stream", I),
    "fea_pcg_direction_f64f32": ("P z32, P p_in, P p_out, P pid, P ktab, I ntab, P scalars, P part, I B, I H, I W, "
                                 "I ld, LL bstride, I ld32, LL bstride32, P stream", I),
    "fea_pcg_update_f64f32": ("P p, P x, P r, P r32, P pid, P ktab, I ntab, P scalars, P sb, P part, I B, I H, I W, "
                              "I ld, LL bstride, I ld32, LL bstride32, P stream", I),
    "fea_stencil_weight_grad_ws_bytes_f32": ("I ntab, I B, I H, I W", ctypes.c_size_t),
    "fea_stencil_weight_grad_ws_bytes_f64": ("I ntab, I B, I H, I W", ctypes.c_size_t),
    "fea_transfer_weight_grad_ws_bytes_f32": ("I C, I B, I Hc, I Wc", ctypes.c_size_t),
    "fea_transfer_weight_grad_ws_bytes_f64": ("I C, I B, I Hc, I Wc", ctypes.c_size_t),
}
# the full-multigrid transfers, declared in include/feanet_fmg.h (typed pairs, the field syntax of _SIGS;
# tests/test_fmg_host.py compares this table with that header)
_FMG = {
    "fmg_prolong": "P u, P ec, P out, I B, I H, I W, I ld, LL bstride, I ldc, LL bstridec, I order, P stream",
    "fmg_restrict": "P f, P fc, I B, I H, I W, I ld, LL bstride, I ldc, LL bstridec, P stream",
    "fmg_boundary": "P bc, LL bc_bstride, I stride, P dst, I B, I H, I W, I ld, LL bstride, P stream",
}
# the two-material set-up from an element phase image, declared in include/feanet_phase.h (dtype-free entry points,
# full names as in _EXTRA, all returning int; tests/test_phase_host.py compares this table with that header)
_PHASE = {
    "fea_phase_pattern_map": "P phase, LL ldp, I He, I We, P pid, LL ldpid, P stream",
    "fea_phase_coarsen": "P fine, LL ldf, I He, I We, P coarse, LL ldc, I min_count, P stream",
}
# the element flux fields and sums, declared in include/feanet_flux.h (tests/test_flux_host.py compares this table
# with that header): "flux" a typed pair in the field syntax of _SIGS, the fea_* names dtype-free entry points as in
# _EXTRA, with their return types in _FLUX_RES
_FLUX = {
    "flux": "P u, P phase, LL ldp, D k0, D k1, D h, P q, LL ldq, LL cstride, LL qbstride, P part, I B, I H, I W, "
            "I ld, LL bstride, P stream",
    "fea_flux_parts": "I H, I W, I elem_size",
    "fea_flux_final": "P part, LL per, P sums, I B, P stream",
}
_FLUX_RES = {"fea_flux_parts": LL, "fea_flux_final": I}
# the bilinear energy forms and their element densities, declared in include/feanet_energy.h (tests/
# test_energy_host.py compares this table with that header), in the form of _FLUX / _FLUX_RES
_ENERGY = {
    "energy": "P u, P v, P phase, LL ldp, P dens, LL ldd, LL cstride, LL dbstride, P part, I B, I H, I W, I ld, "
              "LL ubstride, LL vbstride, P stream",
    "fea_energy_parts": "I H, I W, I elem_size",
    "fea_energy_final": "P part, LL per, P sums, I B, P stream",
}
_ENERGY_RES = {"fea_energy_parts": LL, "fea_energy_final": I}
# the torus (periodic cell) multigrid kernels, declared in include/feanet_periodic.h (tests/test_periodic_host.py
# compares this table with that header), in the form of _FLUX / _FLUX_RES
_PERIODIC = {
    "per_sweep": "P u, P f, P out, P pid, LL ldp, P ktab, P omd, I B, I m, I n, I ld, LL bstride, P stream",
    "per_residual_restrict": "P u, P f, P fc, P pid, LL ldp, P ktab, I B, I m, I n, I ld, LL bstride, I ldc, "
                             "LL bstridec, P stream",
    "per_prolong_add": "P ec, P u, I B, I m, I n, I ld, LL bstride, I ldc, LL bstridec, P stream",
    "per_apply": "P p, P y, P part, P pid, LL ldp, P ktab, I B, I m, I n, I ld, LL bstride, P stream",
    "per_reduce": "P a, P b, P part, I B, I m, I n, I ld, LL bstride, P stream",
    "fea_per_parts": "I m, I n, I elem_size",
    "fea_per_final": "P part, LL per, P sums, I count, P stream",
}
_PERIODIC_RES = {"fea_per_parts": LL, "fea_per_final": I}
# the element-coefficient-field kernels on the torus, declared in include/feanet_coef.h (tests/test_coef_host.py
# compares this table with that header), in the form of _PERIODIC / _PERIODIC_RES; every entry point is a typed pair,
# so the table of dtype-free results is empty (the partial-sum count and the final sum are _PERIODIC's)
_COEF = {
    "coef_sweep": "P u, P f, P out, P k, LL ldk, D omega, I B, I m, I n, I ld, LL bstride, P stream",
    "coef_apply": "P p, P y, P part, P k, LL ldk, I B, I m, I n, I ld, LL bstride, P stream",
    "coef_residual_restrict": "P u, P f, P fc, P k, LL ldk, I B, I m, I n, I ld, LL bstride, I ldc, LL bstridec, "
                              "P stream",
    "coef_coarsen": "P k, LL ldk, P kc, LL ldkc, I m, I n, I rule, P stream",
}
_COEF_RES = {}
# as lists of "TYPE param" fields: len() of an entry is its number of C arguments
_ENERGY = {name: sig.split(", ") for name, sig in _ENERGY.items()}
_PERIODIC = {name: sig.split(", ") for name, sig in _PERIODIC.items()}
_COEF = {name: sig.split(", ") for name, sig in _COEF.items()}
_FLUX = {name: sig.split(", ") for name, sig in _FLUX.items()}
_FMG = {name: sig.split(", ") for name, sig in _FMG.items()}
_PHASE = {name: sig.split(", ") for name, sig in _PHASE.items()}
_SIGS = {name: sig.split(", ") for name, sig in _SIGS.items()}
_EXTRA = {name: (sig.split(", ") if sig else [], res) for name, (sig, res) in _EXTRA.items()}

_lib = None


def _argtypes(sig, S=None):
    return [S if t == "S" else _CTYPES[t] for t in (p.split()[0] for p in sig)]


_NAMES = {}  # launch name -> parameter names in C-ABI order, without the trailing stream


def _names(name):
    """Parameter names of a launch record's entry point: a typed pair's base name, or a dtype-free fea_<name>."""
    if name not in _NAMES:
        sig = _SIGS.get(name) or _FMG.get(name) or _PHASE.get("fea_" + name) or _FLUX.get(name) or \
            _FLUX.get("fea_" + name) or _ENERGY.get(name) or _ENERGY.get("fea_" + name) or \
            _PERIODIC.get(name) or _PERIODIC.get("fea_" + name) or \
            _COEF.get(name) or _COEF.get("fea_" + name) or \
            _EXTRA.get("fea_" + name, ([],))[0]
        names = [p.split()[1] for p in sig]
        if names[-1:] != ["stream"]:
            raise TypeError(f"feanet_amd: no entry point fea_{name} that launches on a stream")
        _NAMES[name] = tuple(names[:-1])
    return _NAMES[name]


def launch(name, **kw):
    """A launch record (name, args): args the positional tuple of fea_<name>'s parameters in header order, without
    the stream, every one given by name (a NULL pointer is written u=None)."""
    names = _names(name)
    for n in names:
        if n not in kw:
            raise TypeError(f"feanet_amd: fea_{name} launch lacks parameter {n!r}")
    if len(kw) != len(names):
        raise TypeError(f"feanet_amd: fea_{name} has no parameter {sorted(set(kw) - set(names))[0]!r}")
    return (name, tuple(kw[n] for n in names))


def arg(launch, pname):
    """Value of parameter `pname` in a launch record."""
    name, args = launch
    names = _names(name)
    if pname not in names:
        raise TypeError(f"feanet_amd: fea_{name} has no parameter {pname!r}")
    return args[names.index(pname)]


def replace(launch, **kw):
    """The launch record with the given parameters changed."""
    name, args = launch
    names = _names(name)
    args = list(args)
    for n, v in kw.items():
        if n not in names:
            raise TypeError(f"feanet_amd: fea_{name} has no parameter {n!r}")
        args[names.index(n)] = v
    return (name, tuple(args))


def exported_symbols():
    """Every symbol the library must export (== every function declared in feanet_hip.h)."""
    names = list(_EXTRA)
    for base in _SIGS:
        names += [f"fea_{base}_f32", f"fea_{base}_f64"]
    return names


def fmg_exported_symbols():
    """Every symbol declared in feanet_fmg.h."""
    return [f"fea_{base}_{suf}" for base in _FMG for suf in ("f32", "f64")]


def phase_exported_symbols():
    """Every symbol declared in feanet_phase.h."""
    return list(_PHASE)


def flux_exported_symbols():
    """Every symbol declared in feanet_flux.h."""
    names = []
    for n in _FLUX:
        names += [n] if n.startswith("fea_") else [f"fea_{n}_f32", f"fea_{n}_f64"]
    return names


def energy_exported_symbols():
    """Every symbol declared in feanet_energy.h."""
    names = []
    for n in _ENERGY:
        names += [n] if n.startswith("fea_") else [f"fea_{n}_f32", f"fea_{n}_f64"]
    return names


def periodic_exported_symbols():
    """Every symbol declared in feanet_periodic.h."""
    names = []
    for n in _PERIODIC:
        names += [n] if n.startswith("fea_") else [f"fea_{n}_f32", f"fea_{n}_f64"]
    return names


def coef_exported_symbols():
    """Every symbol declared in feanet_coef.h."""
    names = []
    for n in _COEF:
        names += [n] if n.startswith("fea_") else [f"fea_{n}_f32", f"fea_{n}_f64"]
    return names


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB):
        raise RuntimeError(f"feanet_amd: {LIB} is missing; run `python -m feanet_amd.build` "
                           "(there is no CPU fallback for the HIP path)")
    L = ctypes.CDLL(LIB)  # (A/B builds of tools/lab replace the module attribute LIB: tools/lab/with_lib.py)
    lab = os.path.abspath(LIB) != os.path.abspath(_IN_TREE)  # an older lab build may lack newer entry points

    def sym(name):
        if lab and not hasattr(L, name):
            return None
        return getattr(L, name)
    for name, (sig, res) in _EXTRA.items():
        fn = sym(name)
        if fn is not None:
            fn.argtypes = _argtypes(sig)
            fn.restype = res
    for name, sig in _PHASE.items():
        fn = sym(name)
        if fn is not None:
            fn.argtypes = _argtypes(sig)
            fn.restype = I
    for table, results in ((_FLUX, _FLUX_RES), (_ENERGY, _ENERGY_RES), (_PERIODIC, _PERIODIC_RES),
                           (_COEF, _COEF_RES)):
        for name, res in results.items():
            fn = sym(name)
            if fn is not None:
                fn.argtypes = _argtypes(table[name])
                fn.restype = res
    typed_flux = [(n, sig) for n, sig in _FLUX.items() if n not in _FLUX_RES]
    typed_flux += [(n, sig) for n, sig in _ENERGY.items() if n not in _ENERGY_RES]
    typed_flux += [(n, sig) for n, sig in _PERIODIC.items() if n not in _PERIODIC_RES]
    typed_flux += [(n, sig) for n, sig in _COEF.items() if n not in _COEF_RES]
    for base, sig in list(_SIGS.items()) + list(_FMG.items()) + typed_flux:
        for suf, S in (("f32", F32), ("f64", F64)):
            fn = sym(f"fea_{base}_{suf}")
            if fn is not None:
                fn.argtypes = _argtypes(sig, S)
                fn.restype = I
    if L.fea_abi_version() != ABI_VERSION:
        raise RuntimeError("feanet_amd: libfeanet_hip.so ABI version mismatch; rebuild it")
    _lib = L
    return L


def call(name, dtype, *args):
    """Invoke fea_<name>_{f32,f64}; raise RuntimeError on a nonzero return (FEA_EINVAL or hipError_t)."""
    suf = {torch.float32: "f32", torch.float64: "f64"}.get(dtype)
    if suf is None:
        raise TypeError(f"feanet_amd: unsupported dtype {dtype} (float32/float64 only)")
    fn = getattr(lib(), f"fea_{name}_{suf}")
    rc = fn(*[a.ptr if isinstance(a, PtrArray) else a for a in args])
    if rc != 0:
        what = "invalid arguments" if rc == -1 else f"hipError_t {rc}"
        raise RuntimeError(f"feanet_amd: fea_{name}_{suf} failed ({what})")


def call_raw(name, *args):
    """Invoke a dtype-free entry point fea_<name> (e.g. norm_append); RuntimeError on a nonzero return."""
    rc = getattr(lib(), f"fea_{name}")(*args)
    if rc != 0:
        raise RuntimeError(f"feanet_amd: fea_{name} failed ({'invalid arguments' if rc == -1 else f'hipError_t {rc}'})")


def join_norm_parts(B, H, W, elem_size):
    """Per-sample partial sums the cycle join writes in its deferred-norm mode."""
    return int(lib().fea_mg_join_norm_parts(B, H, W, elem_size))


def mg_layout(H, W, elem_size):
    """(ld, bstride) of the framed layout of an H x W grid."""
    ld = I()
    bs = LL()
    if lib().fea_mg_layout(H, W, elem_size, ctypes.byref(ld), ctypes.byref(bs)) != 0:
        raise ValueError(f"feanet_amd: unsupported level size {H} x {W} (need H, W >= 3)")
    return ld.value, bs.value


TAIL_LDS_LIMIT = 160 * 1024 - 1024


def coarse_tail_lds_bytes(Ht, Wt, nlev, elem_size, multi):
    return int(lib().fea_mg_coarse_tail_lds_bytes(Ht, Wt, nlev, elem_size, int(bool(multi))))


def hjac_tail_lds_bytes(Ht, Wt, nlev, elem_size, multi):
    return int(lib().fea_mg_hjac_tail_lds_bytes(Ht, Wt, nlev, elem_size, int(bool(multi))))


def weight_grad_ws_bytes(C, B, Hc, Wc):
    return int(lib().fea_transfer_weight_grad_ws_bytes_f64(C, B, Hc, Wc))


def stencil_grad_ws_bytes(ntab, B, H, W):
    return int(lib().fea_stencil_weight_grad_ws_bytes_f64(ntab, B, H, W))


def mid_lds_bytes(up, k, TR, TC, elem_size, multi):
    return int(lib().fea_mg_mid_lds_bytes(int(bool(up)), k, TR, TC, elem_size, int(bool(multi))))


def hmid_lds_bytes(up, T, nlayers, elem_size, multi):
    return int(lib().fea_mg_hmid_lds_bytes(int(bool(up)), T, nlayers, elem_size, int(bool(multi))))


class PtrArray:
    """A C array of device pointers (const T* const*) for the mid-level entry points; keeps the
    ctypes array alive as long as the launch plan that holds it."""

    def __init__(self, ptrs):
        self.arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
        self.ptr = ctypes.cast(self.arr, ctypes.c_void_p).value

    def __repr__(self):
        return f"PtrArray({list(self.arr)})"


def norm_workspace_bytes(B, H, W):
    return int(lib().fea_norm_workspace_bytes(B, H, W))
