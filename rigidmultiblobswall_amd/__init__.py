"""MI355X-native blob-mobility engine: RPY + single-wall M.f products and blob-blob forces.

Layout (only what the hot path needs):
  csrc/         HIP kernels (*_kernels.h, pair_*.h) + C ABI in separately compiled units (rmb_internal.h lists them)
                -> librmb_mobility.so
  _lib.py       ctypes binding of include/rmb_mobility.h (no CPU fallback)
  context.py    persistent per-GPU context (resident positions, host + device entry points)
  mobility.py   the reference's mobility/mobility.py function surface, `<impl> = hip`
  forces.py     calc_blob_blob_forces_hip
  potential.py  blobs_potential_hip / compute_total_energy_hip (the many_bodyMCMC energy surface)
  distributed.py  pair / target sharding over torch.distributed (RCCL) + ReplicatedContext for the callers
callers built on the path, each mirroring the reference module of the same role:
  rigid.py             RigidSuspension: saddle-point operator, block-diagonal preconditioner, choice of the solver path
  krylov.py            the lockstep driver, right-preconditioned GMRES and its two static workspaces
  rigid_integrator.py  RigidIntegrator: deterministic / Brownian schemes for rigid multiblobs, deck driver
  rollers.py           RollersIntegrator: single-blob roller schemes, deck driver
  stochastic.py        Lanczos M^{1/2} z (+ dense forcings)
  utilities.py         one-shot mobility / resistance / body_mobility problems, velocity field
  read_input.py, structures.py, dispatch.py   decks, .vertex / .clones / .slip files, backend strings
  __main__.py          python -m rigidmultiblobswall_amd --input-file deck
  mcmc.py              MCMCSampler: Metropolis sampler of rigid-body configurations, python -m rigidmultiblobswall_amd.mcmc deck
  correlation.py       RadialDistribution: g(r) from the HIP pair-distance histogram, python -m rigidmultiblobswall_amd.correlation
  msd.py               MeanSquareDisplacement: 6 x 6 translational-rotational MSD from the HIP lag sweep, python -m rigidmultiblobswall_amd.msd
  scattering.py        IntermediateScattering: S(k), F(k, t), F_s(k, t) from the HIP Fourier sweeps, python -m rigidmultiblobswall_amd.scattering
  bondorder.py         BondOrder: psi_m, g_m(r), C_m(t) from the HIP neighbour and pair-field sweeps, python -m rigidmultiblobswall_amd.bondorder
  clusters.py          Clusters: cluster labels, sizes and size distribution from the HIP union-find sweep, python -m rigidmultiblobswall_amd.clusters
  hydrofunction.py     HydrodynamicFunction: H(k), H_s, H / S from the HIP pair-block quadratic-form sweep, python -m rigidmultiblobswall_amd.hydrofunction
"""
from . import _lib  # noqa: F401
from .context import MobilityContext  # noqa: F401
from . import mobility  # noqa: F401
from . import forces  # noqa: F401

__all__ = ["MobilityContext", "mobility", "forces"]
