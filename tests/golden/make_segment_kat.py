"""Writes tests/golden/segment_kat.json: the literal inputs and expected arrays of the reference's segmentation and map_array
tests (cupyimg/skimage/segmentation/tests/test_boundaries.py, test_join.py, cupyimg/skimage/util/tests/test_map_array.py) and of
the docstring examples of boundaries.py and _join.py, as data, each with its file:line.  Nothing here calls the library or the
reference.  Inputs the reference's tests build with a few NumPy calls are kept as recipes (tests/test_segment_yardstick.py
kat_array turns them into arrays).

    python tests/golden/make_segment_kat.py
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

F, T = False, True

SQUARE_THICK = [[0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                [0, 0, 1, 1, 1, 1, 1, 0, 0, 0],
                [0, 1, 1, 1, 1, 1, 1, 1, 0, 0],
                [0, 1, 1, 0, 0, 0, 1, 1, 0, 0],
                [0, 1, 1, 0, 0, 0, 1, 1, 0, 0],
                [0, 1, 1, 0, 0, 0, 1, 1, 0, 0],
                [0, 1, 1, 1, 1, 1, 1, 1, 0, 0],
                [0, 0, 1, 1, 1, 1, 1, 0, 0, 0],
                [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
SQUARE_OUTLINED = [[0, 2, 2, 2, 2, 2, 2, 2, 0, 0],
                   [2, 2, 1, 1, 1, 1, 1, 2, 2, 0],
                   [2, 1, 1, 1, 1, 1, 1, 1, 2, 0],
                   [2, 1, 1, 2, 2, 2, 1, 1, 2, 0],
                   [2, 1, 1, 2, 0, 2, 1, 1, 2, 0],
                   [2, 1, 1, 2, 2, 2, 1, 1, 2, 0],
                   [2, 1, 1, 1, 1, 1, 1, 1, 2, 0],
                   [2, 2, 1, 1, 1, 1, 1, 2, 2, 0],
                   [0, 2, 2, 2, 2, 2, 2, 2, 0, 0],
                   [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
BOOL_THICK = [[F, F, F, F, F],
              [F, F, T, T, T],
              [F, T, T, T, T],
              [F, T, T, F, F],
              [F, T, T, F, F]]
DOC_LABELS = [[0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
              [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
              [0, 0, 0, 0, 0, 5, 5, 5, 0, 0],
              [0, 0, 1, 1, 1, 5, 5, 5, 0, 0],
              [0, 0, 1, 1, 1, 5, 5, 5, 0, 0],
              [0, 0, 1, 1, 1, 5, 5, 5, 0, 0],
              [0, 0, 0, 0, 0, 5, 5, 5, 0, 0],
              [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
              [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
DOC_THICK = [[0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
             [0, 0, 0, 0, 0, 1, 1, 1, 0, 0],
             [0, 0, 1, 1, 1, 1, 1, 1, 1, 0],
             [0, 1, 1, 1, 1, 1, 0, 1, 1, 0],
             [0, 1, 1, 0, 1, 1, 0, 1, 1, 0],
             [0, 1, 1, 1, 1, 1, 0, 1, 1, 0],
             [0, 0, 1, 1, 1, 1, 1, 1, 1, 0],
             [0, 0, 0, 0, 0, 1, 1, 1, 0, 0],
             [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
DOC_INNER = [[0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
             [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
             [0, 0, 0, 0, 0, 1, 1, 1, 0, 0],
             [0, 0, 1, 1, 1, 1, 0, 1, 0, 0],
             [0, 0, 1, 0, 1, 1, 0, 1, 0, 0],
             [0, 0, 1, 1, 1, 1, 0, 1, 0, 0],
             [0, 0, 0, 0, 0, 1, 1, 1, 0, 0],
             [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
             [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
DOC_OUTER = [[0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
             [0, 0, 0, 0, 0, 1, 1, 1, 0, 0],
             [0, 0, 1, 1, 1, 1, 0, 0, 1, 0],
             [0, 1, 0, 0, 1, 1, 0, 0, 1, 0],
             [0, 1, 0, 0, 1, 1, 0, 0, 1, 0],
             [0, 1, 0, 0, 1, 1, 0, 0, 1, 0],
             [0, 0, 1, 1, 1, 1, 0, 0, 1, 0],
             [0, 0, 0, 0, 0, 1, 1, 1, 0, 0],
             [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
DOC_SMALL = [[0, 0, 0, 0],
             [0, 0, 5, 0],
             [0, 1, 5, 0],
             [0, 0, 5, 0],
             [0, 0, 0, 0]]
DOC_SUBPIXEL = [[0, 0, 0, 0, 0, 0, 0],
                [0, 0, 0, 1, 1, 1, 0],
                [0, 0, 0, 1, 0, 1, 0],
                [0, 1, 1, 1, 0, 1, 0],
                [0, 1, 0, 1, 0, 1, 0],
                [0, 1, 1, 1, 0, 1, 0],
                [0, 0, 0, 1, 0, 1, 0],
                [0, 0, 0, 1, 1, 1, 0],
                [0, 0, 0, 0, 0, 0, 0]]
# test_boundaries.py:136-144: only the positions equal to 1 are compared there (:155)
SUBPIXEL_MARKED = [[0.55, 0.63, 0.72, 0.69, 0.6, 0.55, 0.54],
                   [0.45, 0.58, 0.72, 1.0, 1.0, 1.0, 0.69],
                   [0.42, 0.54, 0.65, 1.0, 0.44, 1.0, 0.89],
                   [0.69, 1.0, 1.0, 1.0, 0.69, 1.0, 0.83],
                   [0.96, 1.0, 0.38, 1.0, 0.79, 1.0, 0.53],
                   [0.89, 1.0, 1.0, 1.0, 0.38, 1.0, 0.16],
                   [0.57, 0.78, 0.93, 1.0, 0.07, 1.0, 0.09],
                   [0.2, 0.52, 0.92, 1.0, 1.0, 1.0, 0.54],
                   [0.02, 0.35, 0.83, 0.9, 0.78, 0.81, 0.87]]

RELABEL_IN = [1, 1, 5, 5, 8, 99, 42]
SEQUENTIAL = [1, 3, 0, 2, 5, 4]


def square_labels():
    return dict(recipe="box", shape=[10, 10], dtype="uint8", box=[[2, 7], [2, 7]], value=1)


def sparse(n, pairs, dtype="int64"):
    return dict(recipe="sparse", n=n, pairs=pairs, dtype=dtype)


def build():
    cases = []

    def add(name, ref, kind, **fields):
        cases.append(dict(name=name, ref=ref, kind=kind, **fields))

    # ---- find_boundaries
    add("square_thick", "test_boundaries.py:11-31", "find_boundaries", labels=square_labels(), kwargs={}, expect=SQUARE_THICK)
    add("bool_thick", "test_boundaries.py:34-49", "find_boundaries", labels=dict(recipe="box", shape=[5, 5], dtype="bool", box=[[2, 5], [2, 5]], value=1),
        kwargs={}, expect=BOOL_THICK)
    add("doc_thick", "boundaries.py:92-110", "find_boundaries", labels=dict(data=DOC_LABELS, dtype="uint8"), kwargs=dict(mode="thick"), expect=DOC_THICK)
    add("doc_inner", "boundaries.py:111-120", "find_boundaries", labels=dict(data=DOC_LABELS, dtype="uint8"), kwargs=dict(mode="inner"), expect=DOC_INNER)
    add("doc_outer", "boundaries.py:121-130", "find_boundaries", labels=dict(data=DOC_LABELS, dtype="uint8"), kwargs=dict(mode="outer"), expect=DOC_OUTER)
    add("doc_subpixel", "boundaries.py:131-147", "find_boundaries", labels=dict(data=DOC_SMALL, dtype="uint8"), kwargs=dict(mode="subpixel"),
        expect=DOC_SUBPIXEL)
    add("doc_bool", "boundaries.py:148-158", "find_boundaries", labels=dict(data=[[F] * 5, [F] * 5, [F, F, T, T, T], [F, F, T, T, T], [F, F, T, T, T]], dtype="bool"),
        kwargs={}, expect=BOOL_THICK)

    # ---- mark_boundaries: the channel mean of the marked image
    zeros = dict(recipe="box", shape=[10, 10], dtype="float64", box=[[0, 0], [0, 0]], value=0)
    add("mark_thick", "test_boundaries.py:52-74", "mark_boundaries_mean", image=zeros, labels=square_labels(),
        kwargs=dict(color=[1, 1, 1], mode="thick"), expect=SQUARE_THICK)
    add("mark_thick_outline", "test_boundaries.py:76-94", "mark_boundaries_mean", image=zeros, labels=square_labels(),
        kwargs=dict(color=[1, 1, 1], outline_color=[2, 2, 2], mode="thick"), expect=SQUARE_OUTLINED)
    add("mark_thick_bool_image", "test_boundaries.py:97-119", "mark_boundaries_mean", image=dict(zeros, dtype="bool"), labels=square_labels(),
        kwargs=dict(color=[1, 1, 1], mode="thick"), expect=SQUARE_THICK)
    add("mark_subpixel_ones", "test_boundaries.py:122-155", "mark_boundaries_ones", image=dict(recipe="legacy_rand_round2", seed=0, shape=[5, 4]),
        labels=dict(data=DOC_SMALL, dtype="uint8"), kwargs=dict(color=[1, 1, 1], mode="subpixel"), expect=SUBPIXEL_MARKED)

    # ---- join_segmentations
    add("join_doc", "test_join.py:8-18 (_join.py:26-35)", "join_segmentations", s1=dict(data=[[0, 0, 1, 1], [0, 2, 1, 1], [2, 2, 2, 1]], dtype="int64"),
        s2=dict(data=[[0, 1, 1, 0], [0, 1, 1, 0], [0, 1, 1, 1]], dtype="int64"), expect=[[0, 1, 3, 2], [0, 5, 3, 2], [4, 5, 5, 3]])
    add("join_shapes", "test_join.py:20-23", "join_segmentations", s1=dict(data=[[0, 0, 1, 1], [0, 2, 1, 1], [2, 2, 2, 1]], dtype="int64"),
        s2=dict(data=[[0, 0, 1, 1], [0, 2, 2, 1]], dtype="int64"), raises="ValueError")

    # ---- relabel_sequential: relabeled, dense forward map, dense inverse map
    fw1 = sparse(100, [[1, 1], [5, 2], [8, 3], [42, 4], [99, 5]])
    fw5 = sparse(100, [[1, 5], [5, 6], [8, 7], [42, 8], [99, 9]])
    inv5 = [0, 0, 0, 0, 0, 1, 5, 8, 42, 99]
    add("relabel_offset1", "test_join.py:31-45 (_join.py:94-112)", "relabel_sequential", labels=dict(data=RELABEL_IN, dtype="int64"), offset=1,
        relabeled=[1, 1, 2, 2, 3, 5, 4], forward=fw1, inverse=[0, 1, 5, 8, 42, 99])
    add("relabel_offset5", "test_join.py:48-62 (_join.py:117-119)", "relabel_sequential", labels=dict(data=RELABEL_IN, dtype="int64"), offset=5,
        relabeled=[5, 5, 6, 6, 7, 9, 8], forward=fw5, inverse=inv5)
    add("relabel_offset5_with0", "test_join.py:65-79", "relabel_sequential", labels=dict(data=RELABEL_IN + [0], dtype="int64"), offset=5,
        relabeled=[5, 5, 6, 6, 7, 9, 8, 0], forward=fw5, inverse=inv5)
    add("relabel_uint8", "test_join.py:82-96", "relabel_sequential", labels=dict(data=RELABEL_IN + [0], dtype="uint8"), offset=5,
        relabeled=[5, 5, 6, 6, 7, 9, 8, 0], forward=fw5, inverse=inv5, dtypes=["uint8", "uint8", "uint8"])
    imax = 2 ** 31 - 1
    add("relabel_signed_overflow", "test_join.py:99-107", "relabel_sequential", labels=dict(data=[0, 1, 99, 42, 42], dtype="int32"), offset=imax,
        relabeled=[0, imax, imax + 2, imax + 1, imax + 1], dtypes=["uint32", "uint32", "int32"])
    add("relabel_very_large", "test_join.py:110-114", "relabel_sequential", labels=dict(data=[0, 1, 2 ** 63 - 1, 42, 42], dtype="int64"),
        offset=2 ** 63 - 1, relabeled_max=2 ** 63 + 1)
    for dtype in ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64"):
        add("relabel_stable_" + dtype, "test_join.py:117-138", "relabel_sequential", labels=dict(data=RELABEL_IN + [0], dtype=dtype), offset=1,
            relabeled=[1, 1, 2, 2, 3, 5, 4, 0], dtypes=[dtype] * 3)
        add("relabel_stable_sequential_" + dtype, "test_join.py:117-138", "relabel_sequential", labels=dict(data=SEQUENTIAL, dtype=dtype), offset=1,
            relabeled=SEQUENTIAL, dtypes=[dtype] * 3)
    add("relabel_uint8_overflow", "test_join.py:141-149", "relabel_sequential", labels=dict(data=SEQUENTIAL, dtype="uint8"), offset=254,
        relabeled=[254, 256, 0, 255, 258, 257], dtypes=["uint16", "uint16", "uint8"])
    add("relabel_negative", "test_join.py:152-155", "relabel_sequential", labels=dict(data=[1, 1, 5, -5, 8, 99, 42, 0], dtype="int64"), offset=1,
        raises="ValueError")
    for offset in (0, -3):
        for tag, data in (("", RELABEL_IN + [0]), ("_sequential", SEQUENTIAL)):
            add("relabel_offset_{}{}".format(offset, tag).replace("-", "m"), "test_join.py:158-166", "relabel_sequential", labels=dict(data=data, dtype="int64"),
                offset=offset, raises="ValueError")
    for offset in (1, 5):
        for with0 in (F, T):
            for starts in (F, T):
                data = SEQUENTIAL if with0 else [1, 3, 2, 5, 4]
                given = [v + offset - 1 if starts and v > 0 else v for v in data]
                want = given if starts else [v + offset - 1 if v > 0 else 0 for v in data]
                add("relabel_already_sequential_{}_{}_{}".format(offset, int(with0), int(starts)), "test_join.py:169-187", "relabel_sequential",
                    labels=dict(data=given, dtype="int64"), offset=offset, relabeled=want)
    add("relabel_float", "test_join.py:190-193", "relabel_sequential", labels=dict(data=[0, 2, 2, 1, 1, 8], dtype="float64"), offset=1, raises="TypeError")
    add("arraymap_len", "test_join.py:203-209", "arraymap_len", labels=dict(data=RELABEL_IN + [0], dtype="int64"), forward_len=100, inverse_len=6)

    # ---- map_array's argument errors
    add("map_array_out_shape", "test_map_array.py:7-13", "map_array_raises", shape=[24, 25], out_shape=[24, 24], out_step=[1, 1], raises="ValueError")
    add("map_array_out_strided", "test_map_array.py:16-22", "map_array_raises", shape=[24, 25], out_shape=[72, 50], out_step=[3, 2], raises="ValueError")
    add("arraymap_long_str", "test_map_array.py:25-30", "arraymap_str_lines", nvalues=40, lines=6)
    return dict(source="cupyimg/skimage/segmentation/tests/test_boundaries.py, test_join.py, cupyimg/skimage/util/tests/test_map_array.py, "
                       "docstrings of boundaries.py and _join.py", cases=cases)


def text():
    return json.dumps(build(), indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(os.path.join(HERE, "segment_kat.json"), "w") as f:
        f.write(text())
