"""skimage.measure.regionprops / regionprops_table on device arrays (reference: cupyimg/skimage/measure/_regionprops.py).

The reference copies the label image to the host for SciPy's find_objects and then builds one Python object per region, each
property of which costs several small launches.  Here a call fills tables with one row per label (csrc/regionprops.hip):

    rp_extent_kernel    one sweep over the labels: voxel count, bounding box, sum of the indices (integer atomics, exact)
    rp_centres_kernel   box origin and centroid per region
    rp_moments_kernel   one sweep: the (4,) * ndim raw and central moment tables (double atomics)
    rp_finish_kernel    one thread per region: every derived column, in the reference's operation order

The number of launches does not depend on the number of regions.  `regionprops_table` returns device columns; `regionprops`
returns lazy RegionProperties served from one host copy of the tables.

Deviations from the reference: `min_intensity` / `max_intensity` keep the intensity dtype (the reference's table casts them to
int) and follow this library's NaN rule for extrema; `cache=` is accepted and has no effect; float16 intensity
is computed in float32; object columns of a table ("slice", "image", "intensity_image") are host object arrays; iterating a
region yields the supported properties only.  `coords`, the convex, filled, perimeter, Euler and Feret properties,
`extra_properties` and multichannel intensity images raise NotImplementedError before anything is queued.
"""
import ctypes
import itertools
from warnings import warn

import numpy as np

from ... import core
from ...scipy.ndimage import _support as S
from ...scipy.ndimage import measurements as _m

__all__ = ["regionprops", "regionprops_table", "RegionProperties", "PROPS", "COL_DTYPES", "OBJECT_COLUMNS"]

PROPS = {
    "Area": "area",
    "BoundingBox": "bbox",
    "BoundingBoxArea": "bbox_area",
    "CentralMoments": "moments_central",
    "Centroid": "centroid",
    "ConvexArea": "convex_area",
    "ConvexImage": "convex_image",
    "Coordinates": "coords",
    "Eccentricity": "eccentricity",
    "EquivDiameter": "equivalent_diameter",
    "EulerNumber": "euler_number",
    "Extent": "extent",
    "FeretDiameterMax": "feret_diameter_max",
    "FilledArea": "filled_area",
    "FilledImage": "filled_image",
    "HuMoments": "moments_hu",
    "Image": "image",
    "InertiaTensor": "inertia_tensor",
    "InertiaTensorEigvals": "inertia_tensor_eigvals",
    "IntensityImage": "intensity_image",
    "Label": "label",
    "LocalCentroid": "local_centroid",
    "MajorAxisLength": "major_axis_length",
    "MaxIntensity": "max_intensity",
    "MeanIntensity": "mean_intensity",
    "MinIntensity": "min_intensity",
    "MinorAxisLength": "minor_axis_length",
    "Moments": "moments",
    "NormalizedMoments": "moments_normalized",
    "Orientation": "orientation",
    "Perimeter": "perimeter",
    "CroftonPerimeter": "perimeter_crofton",
    "Slice": "slice",
    "Solidity": "solidity",
    "WeightedCentralMoments": "weighted_moments_central",
    "WeightedCentroid": "weighted_centroid",
    "WeightedHuMoments": "weighted_moments_hu",
    "WeightedLocalCentroid": "weighted_local_centroid",
    "WeightedMoments": "weighted_moments",
    "WeightedNormalizedMoments": "weighted_moments_normalized",
}

OBJECT_COLUMNS = {"image", "coords", "convex_image", "slice", "filled_image", "intensity_image"}

COL_DTYPES = {
    "area": int,
    "bbox": int,
    "bbox_area": int,
    "moments_central": float,
    "centroid": float,
    "convex_area": int,
    "convex_image": object,
    "coords": object,
    "eccentricity": float,
    "equivalent_diameter": float,
    "euler_number": int,
    "extent": float,
    "feret_diameter_max": float,
    "filled_area": int,
    "filled_image": object,
    "moments_hu": float,
    "image": object,
    "inertia_tensor": float,
    "inertia_tensor_eigvals": float,
    "intensity_image": object,
    "label": int,
    "local_centroid": float,
    "major_axis_length": float,
    "max_intensity": int,
    "mean_intensity": float,
    "min_intensity": int,
    "minor_axis_length": float,
    "moments": float,
    "moments_normalized": float,
    "orientation": float,
    "perimeter": float,
    "perimeter_crofton": float,
    "slice": object,
    "solidity": float,
    "weighted_moments_central": float,
    "weighted_centroid": float,
    "weighted_moments_hu": float,
    "weighted_local_centroid": float,
    "weighted_moments": float,
    "weighted_moments_normalized": float,
}

PROP_VALS = set(PROPS.values())

_UNSUPPORTED = ("coords", "convex_area", "convex_image", "solidity", "feret_diameter_max", "filled_area", "filled_image",
                "euler_number", "perimeter", "perimeter_crofton")
_ONLY_2D = ("eccentricity", "moments_hu", "orientation", "weighted_moments_hu")
_INTENSITY = ("intensity_image", "max_intensity", "mean_intensity", "min_intensity", "weighted_moments",
              "weighted_moments_central", "weighted_centroid", "weighted_local_centroid", "weighted_moments_hu",
              "weighted_moments_normalized")
SUPPORTED = tuple(sorted(PROP_VALS.difference(_UNSUPPORTED)))


def _cols(ndim):
    """offsets of the derived table's columns: RpCols of csrc/regionprops.hip"""
    t = 4 ** ndim
    c = {"bbox_area": 0, "extent": 1, "equivalent_diameter": 2, "centroid": 3}
    c["local_centroid"] = c["centroid"] + ndim
    c["moments_normalized"] = c["local_centroid"] + ndim
    c["moments_hu"] = c["moments_normalized"] + t
    c["inertia_tensor"] = c["moments_hu"] + 7
    c["inertia_tensor_eigvals"] = c["inertia_tensor"] + ndim * ndim
    c["major_axis_length"] = c["inertia_tensor_eigvals"] + ndim
    c["minor_axis_length"] = c["major_axis_length"] + 1
    c["eccentricity"] = c["minor_axis_length"] + 1
    c["orientation"] = c["eccentricity"] + 1
    c["stride"] = c["orientation"] + 1
    return c


def _prop_shape(prop, ndim):
    """shape of a property's value: () for a scalar"""
    if prop in ("bbox",):
        return (2 * ndim,)
    if prop in ("centroid", "local_centroid", "weighted_centroid", "weighted_local_centroid", "inertia_tensor_eigvals"):
        return (ndim,)
    if prop in ("moments", "moments_central", "moments_normalized", "weighted_moments", "weighted_moments_central",
                "weighted_moments_normalized"):
        return (4,) * ndim
    if prop in ("moments_hu", "weighted_moments_hu"):
        return (7,)
    if prop == "inertia_tensor":
        return (ndim, ndim)
    return ()


# where a float property lives: (table, name of its first column in _cols or None for a whole moment table)
_FLOAT_SOURCE = {
    "extent": ("derived", "extent"), "equivalent_diameter": ("derived", "equivalent_diameter"), "centroid": ("derived", "centroid"),
    "local_centroid": ("derived", "local_centroid"), "moments_normalized": ("derived", "moments_normalized"),
    "moments_hu": ("derived", "moments_hu"), "inertia_tensor": ("derived", "inertia_tensor"),
    "inertia_tensor_eigvals": ("derived", "inertia_tensor_eigvals"), "major_axis_length": ("derived", "major_axis_length"),
    "minor_axis_length": ("derived", "minor_axis_length"), "eccentricity": ("derived", "eccentricity"),
    "orientation": ("derived", "orientation"), "moments": ("raw", None), "moments_central": ("central", None),
    "weighted_centroid": ("wderived", "centroid"), "weighted_local_centroid": ("wderived", "local_centroid"),
    "weighted_moments_normalized": ("wderived", "moments_normalized"), "weighted_moments_hu": ("wderived", "moments_hu"),
    "weighted_moments": ("wraw", None), "weighted_moments_central": ("wcentral", None),
}
_NEEDS_CENTRAL = ("moments_normalized", "moments_hu", "inertia_tensor", "inertia_tensor_eigvals", "major_axis_length",
                  "minor_axis_length", "eccentricity", "orientation", "moments_central")
_W_NEEDS_CENTRAL = ("weighted_moments_normalized", "weighted_moments_hu", "weighted_moments_central")


def _check_inputs(label_image, intensity_image, coordinates, extra_properties):
    """the reference's argument checks (regionprops, RegionProperties.__init__) and this library's refusals, on shapes and
    dtypes alone: nothing is uploaded or queued"""
    ndim = label_image.ndim if isinstance(label_image, core.ndarray) else np.ndim(label_image)
    if ndim not in (2, 3):
        raise TypeError("Only 2-D and 3-D images supported.")
    dt = _m._dtype_of(label_image)
    if dt.kind not in "iu":
        if dt.kind == "b":
            raise TypeError("Non-integer image types are ambiguous: use skimage.measure.label to label the connected"
                            "components of label_image,or label_image.astype(np.uint8) to interpret"
                            "the True values as a single label.")
        raise TypeError("Non-integer label_image types are ambiguous")
    if coordinates is not None:
        if coordinates == "rc":
            warn("The coordinates keyword argument to skimage.measure.regionprops is deprecated. All features are now computed "
                 "in rc (row-column) coordinates. Please remove `coordinates=\"rc\"` from all calls to regionprops before "
                 "updating scikit-image.", stacklevel=3, category=FutureWarning)
        else:
            raise ValueError('Values other than "rc" for the "coordinates" argument to skimage.measure.regionprops are no '
                             'longer supported. You should update your code to use "rc" coordinates and stop using the '
                             '"coordinates" argument, or use skimage version 0.15.x or earlier.')
    if extra_properties is not None:
        raise NotImplementedError("extra_properties is not supported: a property is a column of the device tables, not a "
                                  "Python callable per region")
    if intensity_image is not None:
        lshape = tuple(label_image.shape) if isinstance(label_image, core.ndarray) else np.shape(label_image)
        ishape = tuple(intensity_image.shape) if isinstance(intensity_image, core.ndarray) else np.shape(intensity_image)
        if not (ishape[:ndim] == lshape and len(ishape) in (ndim, ndim + 1)):
            raise ValueError("Label and intensity image shapes must match, except for channel (last) axis.")
        if len(ishape) != ndim:
            raise NotImplementedError("multichannel intensity images are not supported")
        idt = _m._dtype_of(intensity_image)
        if idt.kind not in "biuf":
            raise TypeError("the intensity image must be of a real dtype, got {}".format(idt))
    return ndim


def _check_property(prop, ndim, has_intensity):
    if prop in _UNSUPPORTED:
        raise NotImplementedError("Property {} is not implemented".format(prop))
    if prop not in PROP_VALS:
        raise AttributeError("'{}' object has no attribute '{}'".format(RegionProperties, prop))
    if prop in _ONLY_2D and ndim > 2:
        raise NotImplementedError("Property %s is not implemented for 3D images" % prop)
    if prop in _INTENSITY and not has_intensity:
        raise AttributeError("No intensity image specified.")


class _Batch:
    """the tables of one regionprops call: computed once, at the first use, on the device; `host` holds one copy of each"""

    def __init__(self, label_image, intensity_image):
        self.label_image = S.as_device(label_image)
        self.ndim = self.label_image.ndim
        self.labels = _m._as_int_labels(self.label_image)           # C-contiguous int32 / int64 (a strided view is compacted)
        self.intensity = None
        self.intensity_in = None
        if intensity_image is not None:
            self.intensity_in = S.as_device(intensity_image)
            inten = self.intensity_in
            if inten.dtype == np.float16:
                inten = inten.astype(np.float32)
            self.intensity = core.ascontiguousarray(inten)
        self.max_label = 0
        if self.labels.size:
            self.max_label = max(_m._max_label(self.label_image, "regionprops")[1], 0)
        self.dev = {}
        self.host = {}
        self.cols = _cols(self.ndim)
        if self.max_label:          # the cap is per table actually allocated: the moment and derived tables check their own
            _m._check_table_rows(self.max_label, 8 * (1 + 3 * self.ndim), "regionprops")

    # ---- device tables
    def table(self, name):
        if name not in self.dev:
            getattr(self, "_make_" + name)()
        return self.dev[name]

    def _make_ext(self):
        self.dev["ext"] = _m._region_extents(self.labels, self.max_label)

    def _moments(self, weighted, want_raw, want_central):
        R, t = self.max_label, 4 ** self.ndim
        pre = "w" if weighted else ""
        _m._check_table_rows(R, 8 * t, "regionprops (moment table)")
        ext = self.table("ext")
        raw = core.empty((R, t), np.float64) if want_raw or (weighted and want_central) else None
        central = core.empty((R, t), np.float64) if want_central else None
        centres = core.empty((R, 2, self.ndim), np.float64)
        la, ea, ca = self.labels._desc(), ext._desc(), centres._desc()
        ia = self.intensity._desc() if weighted else None
        ra = raw._desc() if raw is not None else None
        ma = central._desc() if central is not None else None
        S.check(S.lib().mi_rp_moments(ctypes.byref(la), ctypes.byref(ia) if weighted else None, ctypes.byref(ea),
                                      ctypes.byref(ra) if raw is not None else None,
                                      ctypes.byref(ma) if central is not None else None, ctypes.byref(ca), None), ValueError)
        if raw is not None:
            self.dev[pre + "raw"] = raw
        if central is not None:
            self.dev[pre + "central"] = central
            self.dev[pre + "centres"] = centres

    def need_moments(self, weighted, want_raw, want_central):
        """accumulate the tables that are wanted and not there yet, in one call (one sweep serves raw and central)"""
        pre = "w" if weighted else ""
        want_raw = want_raw and (pre + "raw") not in self.dev
        want_central = want_central and (pre + "central") not in self.dev
        if weighted and want_central:
            want_raw = True             # the weighted centroid is a quotient of this very raw table: both from one call
        if want_raw or want_central:
            self._moments(weighted, want_raw, want_central)

    def _make_raw(self):
        self.need_moments(False, True, False)

    def _make_central(self):
        self.need_moments(False, False, True)

    def _make_wraw(self):
        self.need_moments(True, True, False)

    def _make_wcentral(self):
        self.need_moments(True, True, True)

    def _finish(self, weighted, with_central):
        pre = "w" if weighted else ""
        stride = self.cols["stride"] if with_central else self.cols["moments_normalized"]       # the short row: no central table
        _m._check_table_rows(self.max_label, 8 * stride, "regionprops (derived table)")
        ext = self.table("ext")
        raw = self.table("wraw") if weighted else None
        central = self.table(pre + "central") if with_central else None
        out = core.empty((self.max_label, stride), np.float64)
        ea, oa = ext._desc(), out._desc()
        ra = raw._desc() if raw is not None else None
        ma = central._desc() if central is not None else None
        S.check(S.lib().mi_rp_finish(ctypes.byref(ea), self.ndim, ctypes.byref(ra) if raw is not None else None,
                                     ctypes.byref(ma) if central is not None else None, ctypes.byref(oa), None), ValueError)
        self.dev[pre + "derived"] = out
        self.dev[pre + "derived_full"] = with_central

    def need_derived(self, weighted, with_central):
        pre = "w" if weighted else ""
        if (pre + "derived") not in self.dev or (with_central and not self.dev[pre + "derived_full"]):
            self._finish(weighted, with_central)
        return self.dev[pre + "derived"]

    def intensity_stat(self, which):
        """(max_label,) device column of min / max / mean intensity per label from the existing labelled reductions"""
        key = "i" + which
        if key not in self.dev:
            index = np.arange(1, self.max_label + 1, dtype=np.int64)
            if which == "mean":
                self.dev[key] = _m.mean(self.intensity, self.labels, index)
            else:
                out, _, scalar, restore, _ = _m._extrema(self.intensity, self.labels, index, False)
                self.dev["imin"] = _m._column(out, 0, scalar, restore, index)
                self.dev["imax"] = _m._column(out, 1, scalar, restore, index)
        return self.dev[key]

    def extremum_dtype(self, a):
        """min / max intensity keep the intensity dtype: float16 was reduced in float32 (exact)"""
        return a.astype(np.float16) if self.intensity_in.dtype == np.float16 else a

    # ---- crops
    def crop(self, label, sl, intensity):
        origin = [s.start for s in sl]
        shape = [s.stop - s.start for s in sl]
        src = None
        if intensity:
            if "crop_src" not in self.dev:
                self.dev["crop_src"] = core.ascontiguousarray(self.intensity_in)
            src = self.dev["crop_src"]
        out = core.empty(shape, src.dtype if intensity else np.bool_)
        la, oa = self.labels._desc(), out._desc()
        sa = src._desc() if intensity else None
        S.check(S.lib().mi_rp_crop(ctypes.byref(la), ctypes.byref(sa) if intensity else None, int(label), S.c_int64s(origin),
                                   ctypes.byref(oa), None), ValueError)
        return out

    # ---- the host copy regionprops serves its attributes from
    def load_host(self):
        """every table of the call, computed (what is not there yet) and read back once"""
        if "derived" in self.host:
            return self.host
        self.need_moments(False, True, True)
        self.need_derived(False, True)
        names = ["raw", "central", "derived"]
        if self.intensity is not None:
            self.need_moments(True, True, True)
            self.need_derived(True, True)
            for which in ("mean", "min"):
                self.intensity_stat(which)
            names += ["wraw", "wcentral", "wderived", "imean", "imin", "imax"]
        for n in names:
            self.host[n] = self.dev[n].get()
            if n in ("imin", "imax"):
                self.host[n] = self.extremum_dtype(self.host[n])
        return self.host


class RegionProperties:
    """One labelled region (skimage.measure.RegionProperties).  Scalar and array attributes are host values served from one
    copy of the call's tables; `image` and `intensity_image` are device arrays, one crop launch each."""

    def __init__(self, slice, label, batch, row):
        self.label = label
        self._slice = slice
        self.slice = slice
        self._batch = batch
        self._row = row
        self._ndim = batch.ndim
        self._cache = {}
        self._label_image = batch.label_image
        self._intensity_image = batch.intensity_in

    def _derived(self, name):
        _check_property(name, self._ndim, self._intensity_image is not None)
        h = self._batch.load_host()
        c = self._batch.cols
        base = {"weighted_centroid": "centroid", "weighted_local_centroid": "local_centroid",
                "weighted_moments_normalized": "moments_normalized", "weighted_moments_hu": "moments_hu"}.get(name, name)
        table = h["wderived" if name.startswith("weighted") else "derived"]
        shape = _prop_shape(name, self._ndim)
        n = int(np.prod(shape)) if shape else 1
        v = table[self._row, c[base]:c[base] + n]
        return v.reshape(shape).copy() if shape else float(v[0])

    area = property(lambda self: int(self._batch.host["ext"][self._row, 0]))

    @property
    def bbox(self):
        return tuple([self.slice[i].start for i in range(self._ndim)] + [self.slice[i].stop for i in range(self._ndim)])

    @property
    def bbox_area(self):
        return int(np.prod([s.stop - s.start for s in self.slice], dtype=np.int64))

    centroid = property(lambda self: tuple(float(v) for v in self._derived("centroid")))
    local_centroid = property(lambda self: tuple(float(v) for v in self._derived("local_centroid")))
    extent = property(lambda self: self._derived("extent"))
    equivalent_diameter = property(lambda self: self._derived("equivalent_diameter"))
    moments_normalized = property(lambda self: self._derived("moments_normalized"))
    moments_hu = property(lambda self: self._derived("moments_hu"))
    inertia_tensor = property(lambda self: self._derived("inertia_tensor"))
    inertia_tensor_eigvals = property(lambda self: self._derived("inertia_tensor_eigvals"))
    major_axis_length = property(lambda self: self._derived("major_axis_length"))
    minor_axis_length = property(lambda self: self._derived("minor_axis_length"))
    eccentricity = property(lambda self: self._derived("eccentricity"))
    orientation = property(lambda self: self._derived("orientation"))
    weighted_centroid = property(lambda self: tuple(float(v) for v in self._derived("weighted_centroid")))
    weighted_local_centroid = property(lambda self: self._derived("weighted_local_centroid"))
    weighted_moments_normalized = property(lambda self: self._derived("weighted_moments_normalized"))
    weighted_moments_hu = property(lambda self: self._derived("weighted_moments_hu"))

    def _table(self, name, prop):
        _check_property(prop, self._ndim, self._intensity_image is not None)
        return self._batch.load_host()[name][self._row].reshape((4,) * self._ndim).copy()

    moments = property(lambda self: self._table("raw", "moments"))
    moments_central = property(lambda self: self._table("central", "moments_central"))
    weighted_moments = property(lambda self: self._table("wraw", "weighted_moments"))
    weighted_moments_central = property(lambda self: self._table("wcentral", "weighted_moments_central"))

    def _stat(self, which, prop):
        _check_property(prop, self._ndim, self._intensity_image is not None)
        return self._batch.load_host()["i" + which][self._row]

    min_intensity = property(lambda self: self._stat("min", "min_intensity"))
    max_intensity = property(lambda self: self._stat("max", "max_intensity"))
    mean_intensity = property(lambda self: self._stat("mean", "mean_intensity"))

    @property
    def image(self):
        if "image" not in self._cache:
            self._cache["image"] = self._batch.crop(self.label, self.slice, False)
        return self._cache["image"]

    @property
    def intensity_image(self):
        if self._intensity_image is None:
            raise AttributeError("No intensity image specified.")
        if "intensity_image" not in self._cache:
            self._cache["intensity_image"] = self._batch.crop(self.label, self.slice, True)
        return self._cache["intensity_image"]

    def __getattr__(self, attr):
        # reached for names without a property, and when a property's own code raised AttributeError
        if attr in _INTENSITY and self.__dict__.get("_intensity_image") is None:
            raise AttributeError("No intensity image specified.")
        if attr in _UNSUPPORTED:
            raise NotImplementedError("Property {} is not implemented".format(attr))
        raise AttributeError("'{}' object has no attribute '{}'".format(type(self), attr))

    def __iter__(self):
        props = set(SUPPORTED)
        if self._intensity_image is None:
            props = props.difference(_INTENSITY)
        if self._ndim > 2:
            props = props.difference(_ONLY_2D)
        return iter(sorted(props))

    def __getitem__(self, key):
        if key in PROPS and key not in PROP_VALS:       # backwards compatibility: the CamelCase names
            key = PROPS[key]
        return getattr(self, key)

    def __eq__(self, other):
        if not isinstance(other, RegionProperties):
            return False
        if set(self) != set(other):
            return False
        for key in self:
            v1, v2 = getattr(self, key), getattr(other, key)
            if isinstance(v1, core.ndarray):
                v1, v2 = v1.get(), (v2.get() if isinstance(v2, core.ndarray) else v2)
            try:
                np.testing.assert_equal(v1, v2)       # so that NaNs are equal
            except AssertionError:
                return False
        return True

    __hash__ = None


def regionprops(label_image, intensity_image=None, cache=True, coordinates=None, *, extra_properties=None):
    """Measure properties of labelled image regions (skimage.measure.regionprops; _regionprops.py:942-1252).

    Returns lazy RegionProperties in ascending label order, labels no voxel carries skipped.  The call itself sweeps the
    labels once (rp_extent_kernel) and reads the extent table back: `label`, `area`, `slice`, `bbox` and `bbox_area` come
    from it.  The first other attribute of any region computes every table of the call on the device and reads them to
    the host once.  `image` and `intensity_image` are device arrays, one crop launch each.  `cache` has no effect."""
    _check_inputs(label_image, intensity_image, coordinates, extra_properties)
    batch = _Batch(label_image, intensity_image)
    if batch.max_label < 1:
        return []
    ext = batch.table("ext").get()
    batch.host["ext"] = ext
    regions = []
    for i, sl in enumerate(_m._slices_of(ext, batch.ndim)):
        if sl is not None:
            regions.append(RegionProperties(sl, i + 1, batch, i))
    return regions


def _column_names(properties, ndim, separator):
    names = []
    for prop in properties:
        shape = _prop_shape(prop, ndim)
        if not shape or prop in OBJECT_COLUMNS:
            names.append((prop, prop, None))
        else:
            for k, ind in enumerate(np.ndindex(shape)):
                names.append((separator.join(map(str, (prop,) + ind)), prop, k))
    return names


def _col_dtype(prop, batch_intensity_dtype):
    if prop in ("min_intensity", "max_intensity"):
        return batch_intensity_dtype
    dt = COL_DTYPES[prop]
    return np.dtype(object) if dt is object else np.dtype(np.int64 if dt is int else np.float64)


def _take_column(table, k):
    """column k of a (K, n) device table as a C-contiguous (K,) array (one strided copy)"""
    return core.ascontiguousarray(table[:, k])


def regionprops_table(label_image, intensity_image=None, properties=("label", "bbox"), *, cache=True, separator="-",
                      extra_properties=None):
    """Region properties as a dictionary of columns (skimage.measure.regionprops_table; _regionprops.py:767-939).

    Column names, their order, the separator rule and the zero-region case (the right names and dtypes, length 0) are the
    reference's.  Integer columns are int64 and float columns float64 device arrays; `min_intensity` / `max_intensity` keep
    the intensity dtype; object columns are host object arrays.  Only the tables the requested properties need are
    accumulated: two sweeps over the label image at most for the unweighted set, and a handful of launches whatever the
    number of regions.  The device is synchronised for the label maximum and for the number of regions present."""
    ndim = _check_inputs(label_image, intensity_image, None, extra_properties)
    properties = list(properties)
    for prop in properties:
        _check_property(prop, ndim, intensity_image is not None)
    idt = _m._dtype_of(intensity_image) if intensity_image is not None else None
    names = _column_names(properties, ndim, separator)
    batch = _Batch(label_image, intensity_image)
    present = None
    if batch.max_label >= 1:
        ext = batch.table("ext")
        present = core.flatnonzero(_take_column(ext, 0))            # rows of the labels some voxel carries
    if present is None or present.size == 0:
        return {name: (np.empty(0, object) if prop in OBJECT_COLUMNS else core.empty((0,), _col_dtype(prop, idt)))
                for name, prop, _ in names}
    K = present.size
    need = set(properties)
    gathered = {}
    # the moment tables every requested property needs, accumulated together: one sweep serves raw and central
    uw_central = any(p in need for p in _NEEDS_CENTRAL)
    if "moments" in need or uw_central:
        batch.need_moments(False, "moments" in need, uw_central)
    w_central = any(p in need for p in _W_NEEDS_CENTRAL)
    if w_central or any(p in need for p in ("weighted_moments", "weighted_centroid", "weighted_local_centroid")):
        batch.need_moments(True, True, w_central)

    def rows(name):
        """the present rows of a table, gathered once"""
        if name not in gathered:
            if name == "ext":
                t = batch.table("ext")
            elif name in ("raw", "central", "wraw", "wcentral"):
                weighted = name.startswith("w")
                batch.need_moments(weighted, any(p in need for p in (("weighted_moments",) if weighted else ("moments",))),
                                   any(p in need for p in (_W_NEEDS_CENTRAL if weighted else _NEEDS_CENTRAL)))
                t = batch.table(name)
            elif name == "derived":
                t = batch.need_derived(False, any(p in need for p in _NEEDS_CENTRAL))
            else:
                t = batch.need_derived(True, any(p in need for p in _W_NEEDS_CENTRAL))
            gathered[name] = core._take_rows(t, present, t.shape[1])
        return gathered[name]

    ext_host = None
    out = {}
    objects = {}
    for name, prop, k in names:
        if prop in OBJECT_COLUMNS:
            if prop not in objects:
                if ext_host is None:
                    ext_host = rows("ext").get()
                    labels_host = present.get() + 1
                    slices = _m._slices_of(ext_host, ndim)
                col = np.empty(K, object)
                for j in range(K):
                    col[j] = slices[j] if prop == "slice" else batch.crop(int(labels_host[j]), slices[j], prop == "intensity_image")
                objects[prop] = col
            out[name] = objects[prop]
        elif prop == "label":
            out[name] = S.elementwise("add", present, core.ones((K,), np.int64), core.empty((K,), np.int64))
        elif prop == "area":
            out[name] = _take_column(rows("ext"), 0)
        elif prop == "bbox":
            out[name] = _take_column(rows("ext"), 1 + k)
        elif prop == "bbox_area":
            out[name] = _take_column(rows("derived"), batch.cols["bbox_area"]).astype(np.int64)
        elif prop in ("min_intensity", "max_intensity", "mean_intensity"):
            out[name] = core.take(batch.intensity_stat(prop.split("_")[0]), present)
            if prop != "mean_intensity":
                out[name] = batch.extremum_dtype(out[name])
        else:
            table, first = _FLOAT_SOURCE[prop]
            out[name] = _take_column(rows(table), (batch.cols[first] if first else 0) + (k or 0))
    return out
