"""amof_amd -- MI355X-native kernels behind aMOF's pair-distance analysis API.

Drop-in mirrors of the reference's hot-path classes (coudertlab/amof v1.1.0):

    amof.rdf.Rdf                  -> amof_amd.rdf.Rdf
    amof.msd.WindowMsd            -> amof_amd.msd.WindowMsd
    amof.bad.Bad                  -> amof_amd.bad.Bad
    amof.cn.CoordinationNumber    -> amof_amd.cn.CoordinationNumber
    amof.ring.Ring                -> amof_amd.ring.Ring           (primitive ring statistics on the GPU: no RINGS binary)
    amof.coordination.reduce, ReducedTrajectory
                                  -> amof_amd.fragment.Fragments  (building units as connected components of a bond graph,
                                                                   their centres of mass as a trajectory; no zif.py chemistry)

Analyses beyond the reference:

    amof_amd.vanhove.WindowVanHove                self Van Hove function, non-Gaussian parameter
    amof_amd.vanhove_distinct.DistinctVanHove     distinct Van Hove function G_d(r, t) on the same lags
    amof_amd.vacf.VelocityAutocorrelation         velocity autocorrelation function, vibrational density of states
    amof_amd.current_correlation.CurrentCorrelation
                                                  longitudinal and transverse current correlations C_L(q, t), C_T(q, t), their
                                                  spectra, dispersion and sound velocities (also ``amof_amd.CurrentCorrelation``)
    amof_amd.structure_factor.StructureFactor     static structure factor S(q) by direct summation over the
                                                  reciprocal lattice (density_modes: rho_a(k) of one frame)
    amof_amd.intermediate_scattering.IntermediateScattering
                                                  intermediate scattering function F(q, t), coherent and self
    amof_amd.bond_lifetime.BondLifetime           bond survival correlations C(t), S(t) for CoordinationNumber's sets
    amof_amd.bond_reorientation.BondReorientation reorientational correlations C1(t), C2(t) of the same sets' bond vectors
    amof_amd.lindemann.Lindemann                  Lindemann index (bond-length fluctuation) of the same sets per block of frames
    amof_amd.bond_order.BondOrder                 Steinhardt q_l and tetrahedral order parameter of the same sets' shells
    amof_amd.dihedral.Dihedral                    torsion-angle distributions of chains a-b-c-d of bonded atoms (also
                                                  ``amof_amd.Dihedral``)
    amof_amd.pore.Pore                            void fraction, cavity-size histogram and largest included sphere on a grid
                                                  (the reference's Pore wraps the external Zeo++ binary: not its numbers)

All distance arithmetic runs in hand-written HIP kernels (gfx950) behind the C
ABI of ``include/amof_hip.h``; there is no CPU fallback.
"""

__version__ = "0.1.0"

from .frames import Frame, PackedTrajectory, pack_trajectory  # noqa: F401


def __getattr__(name):
    # (on first use: the analysis modules import pandas)
    if name == "Dihedral":
        from .dihedral import Dihedral
        return Dihedral
    if name == "CurrentCorrelation":
        from .current_correlation import CurrentCorrelation
        return CurrentCorrelation
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
