"""skimage.util subset: map_array and ArrayMap (cupyimg/skimage/util/_map_array.py) on the kernels of csrc/segment.hip."""
from ._map_array import ArrayMap, map_array  # noqa: F401

__all__ = ["map_array", "ArrayMap"]
