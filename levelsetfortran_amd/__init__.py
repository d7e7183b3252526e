"""levelsetfortran_amd -- MI355X (gfx950) implementation of the hot path of musheen/LevelSetFortran:
WENO5 Hamilton-Jacobi signed-distance reinitialisation and min/max-flow smoothing on a uniform 3-D
grid, behind the reference's own procedure interface (see levelset.py, include/lsf.h).
"""
from .levelset import (CutCellsReport, cutCellsBand, AdvectBandReport,AdvectPointsReport, AdvectReport, CastReport, CorrectReport, CurvatureReport, EvolveBandCurvReport, EvolveBandReport, ExtendBandReport, ExtendReport, FillReport, LabelReport, LsfError, LsfNaNError, MeasureReport, MeshInfo, ReseedReport, SampleReport, SurfaceInfo, SweepReport, advectField, advectFieldBand, advectNodes, advectPoints, castRays, correctField, curvatureBand, distanceFill, evolveBand, evolveBandCurv, extendField, extendFieldBand, extractSurface, labelBand, measureBand, meshCheck, meshDistance, minmaxFlow, mode_word, narrowBand, peer_selftest,  # noqa: F401
                       phi0Init, RedistanceReport, redistanceBand, reinit, reinit_multi, reinitBand, reseedParticles, samplePoints, seedParticles, stlWrite)
from . import fields  # noqa: F401

__version__ = "0.1.6"
