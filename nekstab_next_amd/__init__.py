"""nekstab_next_amd — MI355X-native Krylov hot path for nekStab (Arnoldi / Krylov–Schur / GMRES).

Host mirror of nekStab's vector/operator/solver interfaces driving hand-written gfx950 HIP kernels
through the C ABI in include/nekkrylov.h (libnekkrylov.so, built in-tree).  See DESIGN.md.
"""
from .layout import NekLayout, box3d_layout, cylinder_layout  # noqa: F401
from .config import GmresConfig, KrylovSchurConfig  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    # GPU-facing modules are imported lazily so that `import nekstab_next_amd` works on a
    # build host without a GPU; they raise loudly on first use if the HIP library or the GPU is absent.
    import importlib

    for mod in ("vector", "operators", "arnoldi", "krylov_schur", "gmres", "newton", "sensitivity", "lapack",
                "comm", "synthetic", "lightkrylov", "drivers", "checkpoint", "fld", "boostconv", "seeds", "fixedp",
                "postproc", "vortex", "forcing", "monitors", "gs", "advdiff", "resolvent", "burgers", "orbit",
                "pressure", "incompressible", "_lib"):
        if name == mod:
            return importlib.import_module(f".{mod}", __name__)
    if name in ("SFD", "TDF"):   # the fixed-point forcing classes (fixedp.py)
        return getattr(importlib.import_module(".fixedp", __name__), name)
    if name in ("Sponge", "SpongeConfig", "BodyForce"):   # the sponge and the body-force assembly (forcing.py)
        return getattr(importlib.import_module(".forcing", __name__), name)
    if name in ("Torque", "TorqueMonitor", "Statistics"):   # the per-step monitors (monitors.py)
        return getattr(importlib.import_module(".monitors", __name__), name)
    if name in ("AdvectionDiffusion", "box_boundary_mask", "mask_from_faces"):   # the model propagator (advdiff.py)
        return getattr(importlib.import_module(".advdiff", __name__), name)
    if name in ("ResolventOperator", "CoupledResolventOperator", "IncompressibleResolventOperator", "pair_context"):   # the time-stepper resolvent over it (resolvent.py)
        return getattr(importlib.import_module(".resolvent", __name__), name)
    if name in ("LinearisedConvection", "ViscousBurgers"):   # the nonlinear flow and its linearisation (burgers.py)
        return getattr(importlib.import_module(".burgers", __name__), name)
    if name in ("OrbitFlow", "OrbitPropagator", "checkpoint_schedule"):   # the time-periodic base flow and its tangent (orbit.py)
        return getattr(importlib.import_module(".orbit", __name__), name)
    if name == "DivergenceFreeProjector":   # the pressure solve of the divergence-free projection (pressure.py)
        return getattr(importlib.import_module(".pressure", __name__), name)
    if name in ("IncompressibleFlow", "LinearisedNavierStokes"):   # the incompressible flow over it (incompressible.py)
        return getattr(importlib.import_module(".incompressible", __name__), name)
    raise AttributeError(name)
