"""feanet_amd — MI355X-native geometric-multigrid hot path of longfish/Multigrid-FEANet.

  feanet_amd.ops          tensor-level HIP operators (KNet apply, Jacobi sweep, R, P, norms)
  feanet_amd.solver       MultigridSolver: fused-kernel V-cycle over framed level buffers
  feanet_amd.pcg          PCGSolver: conjugate gradients preconditioned by that V-cycle
  feanet_amd.flux         element fluxes q = -k grad u, mean flux / gradient, energy of a field (element_flux);
                          energy forms of a pair of fields, split by phase, with their element densities (energy_forms)
  feanet_amd.homogenize   effective_conductivity of a phase image from two load cases (flux or energy route; the
                          energy route with its sensitivities, effective_conductivity_torch for autograd)
  feanet_amd.periodic     PeriodicPCGSolver: the image as a periodic cell, torus multigrid kernels under projected
                          conjugate gradients (effective_conductivity(..., bc="periodic"))
  feanet_amd.coef         CoefPeriodicPCGSolver: the periodic cell with one coefficient per element (matrix-free torus
                          kernels), effective_conductivity_field and its autograd form
  feanet_amd.graphs       GraphCache: eager once, captured as a HIP graph the second time, replayed after
  feanet_amd.mesh_setup  vectorised discretisation tables (pattern maps, stencils)
  FEANet.*                drop-in modules with the reference's names (sibling package)
"""
from . import mesh_setup  # noqa: F401


def __getattr__(name):
    # lazy: importing the package must not require the HIP library (CPU-only test collection)
    if name == "MultigridSolver":
        from .solver import MultigridSolver
        return MultigridSolver
    if name == "PCGSolver":
        from .pcg import PCGSolver
        return PCGSolver
    if name == "PeriodicPCGSolver":
        from .periodic import PeriodicPCGSolver
        return PeriodicPCGSolver
    if name in ("CoefPeriodicPCGSolver", "effective_conductivity_field", "effective_conductivity_field_torch"):
        from . import coef
        return getattr(coef, name)
    if name == "element_flux":
        from .flux import element_flux
        return element_flux
    if name == "energy_forms":
        from .flux import energy_forms
        return energy_forms
    if name == "effective_conductivity_torch":
        from .homogenize import effective_conductivity_torch
        return effective_conductivity_torch
    if name == "effective_conductivity":
        from .homogenize import effective_conductivity
        return effective_conductivity
    if name in ("ops", "solver", "pcg", "_lib", "flux", "homogenize", "periodic", "coef"):
        import importlib
        return importlib.import_module(f".{name}", __name__)
    raise AttributeError(name)
