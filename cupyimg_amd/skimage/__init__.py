"""skimage look-alikes that sit directly on the ndimage hot path (SURVEY.md
section 8a row a15): grey / binary erosion + dilation, gaussian, warp.
Argument massaging only -- all device work happens in cupyimg_amd.scipy.ndimage."""
from . import exposure, feature, filters, measure, morphology, registration, restoration, segmentation, transform, util  # noqa: F401
