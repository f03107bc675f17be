"""NumPy / SciPy transcription of the reference's region measurements for the properties cupyimg_amd supports
(cupyimg/skimage/measure/_regionprops.py, _moments.py; cupyimg/skimage/morphology/misc.py:51-245), one region at a time as the
reference works, plus the rational-arithmetic evaluator behind the bound of the central moment tables.

Nothing here touches the device or reads the reference.  The Hu invariants are written out in the operation order of
skimage's moments_hu, the one rp_finish_kernel follows.
"""
import itertools
import math
from fractions import Fraction

import numpy as np
import scipy.ndimage as sndi

PI = math.pi
COL_DTYPES = {
    "area": int, "bbox": int, "bbox_area": int, "moments_central": float, "centroid": float, "eccentricity": float,
    "equivalent_diameter": float, "extent": float, "moments_hu": float, "image": object, "inertia_tensor": float,
    "inertia_tensor_eigvals": float, "intensity_image": object, "label": int, "local_centroid": float, "major_axis_length": float,
    "max_intensity": int, "mean_intensity": float, "min_intensity": int, "minor_axis_length": float, "moments": float,
    "moments_normalized": float, "orientation": float, "slice": object, "weighted_moments_central": float,
    "weighted_centroid": float, "weighted_moments_hu": float, "weighted_local_centroid": float, "weighted_moments": float,
    "weighted_moments_normalized": float,
}
OBJECT_COLUMNS = {"image", "slice", "intensity_image"}
ONLY_2D = ("eccentricity", "moments_hu", "orientation", "weighted_moments_hu")
INTENSITY = ("intensity_image", "max_intensity", "mean_intensity", "min_intensity", "weighted_moments", "weighted_moments_central",
             "weighted_centroid", "weighted_local_centroid", "weighted_moments_hu", "weighted_moments_normalized")


# ------------------------------------------------------------------ find_objects
def find_objects(labels, max_label=0):
    """scipy.ndimage.find_objects from per-label minima and maxima of the indices"""
    labels = np.asarray(labels)
    if max_label < 1:
        max_label = int(labels.max())
    out = [None] * max(max_label, 0)
    if labels.ndim == 0 or max_label < 1:
        return out
    idx = np.nonzero((labels >= 1) & (labels <= max_label))
    lab = labels[idx].astype(np.int64)
    for v in np.unique(lab):
        sel = lab == v
        out[int(v) - 1] = tuple(slice(int(ax[sel].min()), int(ax[sel].max()) + 1, None) for ax in idx)
    return out


# ------------------------------------------------------------------ _moments.py
def moments_central(image, center, order=3):
    """_moments.py:199-255: one dot per axis, axis 0 first"""
    calc = np.asarray(image).astype(float)
    for dim, dim_length in enumerate(image.shape):
        delta = np.arange(dim_length, dtype=float) - center[dim]
        powers_of_delta = delta[:, np.newaxis] ** np.arange(order + 1)
        calc = np.rollaxis(calc, dim, image.ndim)
        calc = np.dot(calc, powers_of_delta)
        calc = np.rollaxis(calc, -1, dim)
    return calc


def moments(image, order=3):
    return moments_central(image, (0,) * image.ndim, order=order)


def moments_normalized(mu, order=3):
    """_moments.py:258-316"""
    nu = np.zeros_like(mu)
    mu0 = mu.ravel()[0]
    with np.errstate(all="ignore"):
        for powers in itertools.product(range(order + 1), repeat=mu.ndim):
            if sum(powers) < 2:
                nu[powers] = np.nan
            else:
                nu[powers] = mu[powers] / (mu0 ** (sum(powers) / nu.ndim + 1))
    return nu


def moments_hu(nu):
    """Hu's seven invariants in the operation order of skimage.measure.moments_hu (_moments_cy.pyx)"""
    nu = np.asarray(nu, np.float64)
    hu = np.zeros(7, np.float64)
    with np.errstate(all="ignore"):
        t0 = nu[3, 0] + nu[1, 2]
        t1 = nu[2, 1] + nu[0, 3]
        q0 = t0 * t0
        q1 = t1 * t1
        n4 = 4 * nu[1, 1]
        s = nu[2, 0] + nu[0, 2]
        d = nu[2, 0] - nu[0, 2]
        hu[0] = s
        hu[1] = d * d + n4 * nu[1, 1]
        hu[3] = q0 + q1
        hu[5] = d * (q0 - q1) + n4 * t0 * t1
        t0 *= q0 - 3 * q1
        t1 *= 3 * q0 - q1
        q0 = nu[3, 0] - 3 * nu[1, 2]
        q1 = 3 * nu[2, 1] - nu[0, 3]
        hu[2] = q0 * q0 + q1 * q1
        hu[4] = q0 * t0 + q1 * t1
        hu[6] = q1 * t0 - q0 * t1
    return hu


def inertia_tensor(mu):
    """_moments.py:406-460 from the central moments"""
    ndim = mu.ndim
    mu0 = mu[(0,) * ndim]
    result = np.zeros((ndim, ndim))
    corners2 = tuple(2 * np.eye(ndim, dtype=int))
    with np.errstate(all="ignore"):
        d = (np.sum(mu[corners2]) - mu[corners2]) / mu0
        for i in range(ndim):
            result[i, i] = d[i]
        for dims in itertools.combinations(range(ndim), 2):
            mu_index = np.zeros(ndim, dtype=int)
            mu_index[list(dims)] = 1
            result[dims] = -mu[tuple(mu_index)] / mu0
            result.T[dims] = -mu[tuple(mu_index)] / mu0
    return result


def inertia_tensor_eigvals(T):
    """_moments.py:463-511"""
    if not np.all(np.isfinite(T)):
        return np.full(T.shape[0], np.nan)
    eigvals = np.linalg.eigvalsh(T)
    eigvals = np.clip(eigvals, 0, None, out=eigvals)
    return np.asarray(sorted(eigvals, reverse=True))


# ------------------------------------------------------------------ the derived columns from tables
def derived(ndim, area, slc, centroid_sum, mu, eigvals=None, T=None, nu=None):
    """the reference's derived properties of one region from its area, slice, the sums of its indices per axis and its central
    moment table `mu` (_regionprops.py:296-587).  `eigvals`, `T`, `nu`: use these (the device's) instead of computing them, so
    that a column is checked given its inputs."""
    out = {}
    size = 1
    for s in slc:
        size *= s.stop - s.start
    out["bbox_area"] = size
    out["extent"] = area / size
    if ndim == 2:
        out["equivalent_diameter"] = math.sqrt(4 * area / PI)
    else:
        out["equivalent_diameter"] = (2 * ndim * area / PI) ** (1 / ndim)
    if centroid_sum is not None:
        out["centroid"] = tuple(float(s) / float(area) for s in centroid_sum)
        out["local_centroid"] = tuple(float(s - area * sl.start) / float(area) for s, sl in zip(centroid_sum, slc))
    if mu is None:
        return out
    out["moments_normalized"] = moments_normalized(mu) if nu is None else nu
    out["inertia_tensor"] = inertia_tensor(mu) if T is None else T
    out["inertia_tensor_eigvals"] = inertia_tensor_eigvals(out["inertia_tensor"]) if eigvals is None else np.asarray(eigvals)
    ev = out["inertia_tensor_eigvals"]
    with np.errstate(all="ignore"):
        out["major_axis_length"] = 4 * np.sqrt(ev[0])
        out["minor_axis_length"] = 4 * np.sqrt(ev[-1])
        if ndim == 2:
            out["moments_hu"] = moments_hu(out["moments_normalized"])
            l1, l2 = ev
            out["eccentricity"] = 0.0 if l1 == 0 else float(np.sqrt(1 - l2 / l1))
            a, b, b, c = out["inertia_tensor"].ravel()
            if a - c == 0:
                out["orientation"] = -PI / 4.0 if b < 0 else PI / 4.0
            else:
                out["orientation"] = 0.5 * math.atan2(-2 * b, c - a)
    return out


class Region:
    """one region as the reference's RegionProperties computes it: everything from the cropped mask"""

    def __init__(self, slc, label, label_image, intensity_image):
        self.slice, self.label = slc, label
        self.ndim = label_image.ndim
        self.image = label_image[slc] == label
        self.intensity_image = None if intensity_image is None else intensity_image[slc] * self.image
        self.area = int(self.image.sum())
        self.bbox = tuple([s.start for s in slc] + [s.stop for s in slc])
        coords = np.nonzero(self.image)
        sums = [int(c.sum()) + self.area * s.start for c, s in zip(coords, slc)]
        self.moments = moments(self.image.astype(np.uint8))
        ctr = tuple(self.moments[tuple(np.eye(self.ndim, dtype=int))] / self.moments[(0,) * self.ndim])
        self.moments_central = moments_central(self.image.astype(np.uint8), ctr)
        for k, v in derived(self.ndim, self.area, slc, sums, self.moments_central).items():
            setattr(self, k, v)
        self.local_centroid = ctr
        if intensity_image is not None:
            vals = self.intensity_image[self.image]
            # the mean in float64 whatever the intensity dtype (the reference's cp.mean of a float32 crop accumulates in
            # float32; the device divides float64 sums: a documented deviation towards the more accurate value)
            self.min_intensity, self.max_intensity, self.mean_intensity = vals.min(), vals.max(), vals.mean(dtype=np.float64)
            img = self.intensity_image.astype(np.double)
            with np.errstate(all="ignore"):
                self.weighted_moments = moments(img)
                wm = self.weighted_moments
                self.weighted_local_centroid = wm[tuple(np.eye(self.ndim, dtype=int))] / wm[(0,) * self.ndim]
                self.weighted_centroid = tuple(idx + s.start for idx, s in zip(self.weighted_local_centroid, slc))
                self.weighted_moments_central = moments_central(img, self.weighted_local_centroid)
                self.weighted_moments_normalized = moments_normalized(self.weighted_moments_central)
                if self.ndim == 2:
                    self.weighted_moments_hu = moments_hu(self.weighted_moments_normalized)


def regionprops(label_image, intensity_image=None):
    label_image = np.asarray(label_image)
    if label_image.ndim not in (2, 3):
        raise TypeError("Only 2-D and 3-D images supported.")
    if label_image.dtype.kind not in "iu":
        raise TypeError("Non-integer label_image types are ambiguous")
    regions = []
    objects = find_objects(label_image) if label_image.size and label_image.max() > 0 else []
    for i, sl in enumerate(objects):
        if sl is not None:
            regions.append(Region(sl, i + 1, label_image, None if intensity_image is None else np.asarray(intensity_image)))
    return regions


def prop_shape(prop, ndim):
    if prop == "bbox":
        return (2 * ndim,)
    if prop in ("centroid", "local_centroid", "weighted_centroid", "weighted_local_centroid", "inertia_tensor_eigvals"):
        return (ndim,)
    if "moments" in prop and "hu" not in prop:
        return (4,) * ndim
    if prop.endswith("moments_hu"):
        return (7,)
    if prop == "inertia_tensor":
        return (ndim, ndim)
    return ()


def column_names(properties, ndim, separator="-"):
    """[(column name, property, flat index or None)] in the reference's order (_props_to_dict, :723-764)"""
    names = []
    for prop in properties:
        shape = prop_shape(prop, ndim)
        if not shape or prop in OBJECT_COLUMNS:
            names.append((prop, prop, None))
        else:
            for k, ind in enumerate(np.ndindex(shape)):
                names.append((separator.join(map(str, (prop,) + ind)), prop, k))
    return names


def regionprops_table(label_image, intensity_image=None, properties=("label", "bbox"), separator="-", keep_intensity_dtype=True):
    """the reference's table as host arrays: int columns int64, float columns float64, object columns object; the zero-region
    case has the right names and dtypes and length 0 (:917-937).  keep_intensity_dtype: min / max intensity in the intensity's
    dtype (this library's documented deviation) instead of the reference's cast to int."""
    label_image = np.asarray(label_image)
    regions = regionprops(label_image, intensity_image)
    ndim = label_image.ndim
    out = {}
    for name, prop, k in column_names(properties, ndim, separator):
        dt = COL_DTYPES[prop]
        if prop in ("min_intensity", "max_intensity") and keep_intensity_dtype:
            dtype = np.asarray(intensity_image).dtype
        else:
            dtype = np.dtype(object) if dt is object else np.dtype(np.int64 if dt is int else np.float64)
        col = np.empty(len(regions), dtype)
        for j, r in enumerate(regions):
            v = getattr(r, prop)
            col[j] = v if k is None else np.asarray(v).ravel()[k]
        out[name] = col
    return out


# ------------------------------------------------------------------ the bound of the central tables
def exact_central(weights, center):
    """(exact, sumabs): per entry of the (4,) * ndim table the exact value of sum w prod_d (x_d - c_d)^p_d and the sum of the
    terms' magnitudes, in rational arithmetic, for the float64 centre `center` and the weights `weights` (the region's mask or
    intensity crop; zeros contribute nothing) taken as the exact values of their float64 conversions"""
    weights = np.asarray(weights)
    ndim = weights.ndim
    c = [Fraction(float(v)) for v in center]
    pw = [[[(Fraction(i) - c[d]) ** p for p in range(4)] for i in range(weights.shape[d])] for d in range(ndim)]
    exact = np.empty((4,) * ndim, object)
    sumabs = np.empty((4,) * ndim, object)
    exact.fill(Fraction(0))
    sumabs.fill(Fraction(0))
    for idx in zip(*np.nonzero(weights)):
        w = Fraction(float(weights[idx]))
        for powers in itertools.product(range(4), repeat=ndim):
            t = w
            for d in range(ndim):
                t *= pw[d][idx[d]][powers[d]]
            exact[powers] += t
            sumabs[powers] += abs(t)
    return exact, sumabs


def central_bound(area, sumabs):
    """(area + 16) 2^-53 sum|term| per entry: area - 1 roundings of the sum in any order, 16 for the powers, the products and
    the conversions"""
    return np.vectorize(lambda s: (area + 16) * Fraction(1, 2 ** 53) * s, otypes=[object])(sumabs)


def within_central_bound(got, weights, center, area):
    """largest |got - exact| / bound over the table's entries (0 / 0 counts as 0); <= 1 means within the bound"""
    exact, sumabs = exact_central(weights, center)
    bound = central_bound(area, sumabs)
    worst = 0.0
    for powers in itertools.product(range(4), repeat=np.ndim(weights)):
        err = abs(Fraction(float(got[powers])) - exact[powers])
        if err == 0:
            continue
        if bound[powers] == 0:
            return float("inf")
        worst = max(worst, float(err / bound[powers]))
    return worst


def central_sumabs(weights, center):
    """float64 estimate of sum|term| per entry of the central table: the same dots over |w| and |delta|^p (every factor is
    non-negative, so the estimate is within (area + 16) 2^-53 of itself of the rational sum)"""
    calc = np.abs(np.asarray(weights).astype(float))
    for dim, dim_length in enumerate(calc.shape):
        delta = np.abs(np.arange(dim_length, dtype=float) - center[dim])
        calc = np.rollaxis(calc, dim, calc.ndim)
        calc = np.dot(calc, delta[:, np.newaxis] ** np.arange(4))
        calc = np.rollaxis(calc, -1, dim)
    return calc


def ulp_distance(a, b):
    """largest distance in units in the last place between two float64 arrays (NaN against NaN counts as 0)"""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    both_nan = np.isnan(a) & np.isnan(b)
    if np.any(np.isnan(a) != np.isnan(b)):
        return float("inf")
    ia, ib = a.view(np.int64).copy(), b.view(np.int64).copy()
    ia[ia < 0] = np.int64(-2 ** 63) - ia[ia < 0]
    ib[ib < 0] = np.int64(-2 ** 63) - ib[ib < 0]
    d = np.abs(ia.astype(object) - ib.astype(object))
    d[both_nan] = 0
    return int(d.max()) if d.size else 0


# ------------------------------------------------------------------ misc.py
def remove_small_objects(ar, min_size=64, connectivity=1):
    ar = np.asarray(ar)
    out = ar.copy()
    if min_size == 0:
        return out
    if out.dtype == bool:
        ccs = sndi.label(ar, sndi.generate_binary_structure(ar.ndim, connectivity))[0]
    else:
        ccs = out
    sizes = np.bincount(ccs.ravel().astype(np.int64))
    out[(sizes < min_size)[ccs]] = 0
    return out


def remove_small_holes(ar, area_threshold=64, connectivity=1):
    out = np.logical_not(np.asarray(ar))
    out = remove_small_objects(out, area_threshold, connectivity)
    return np.logical_not(out)
