"""What GeometryCodec's front end (stage, keys, sorted / distinct) asks of the library, call by call, and what a call
with nothing to code returns.

The C entry points of a call, in order, with every argument that is a plain number: recorded through a proxy in place
of geo.rt.lib and compared with lists recorded once, with this proxy and these inputs, on the commit before the front
ends of compress and distortion became one (the attribute cases: on the commit before a call's attribute settings
became one record, runtime.AttrCoding, which guards the dispatch among the nine encode entry points).  torch's own launches (cat, the lod mask, zeros, full) do not pass the
proxy.  The blobs themselves are held to the oracle and to the numpy restatements by the other geometry tests.
"""
import ctypes as C

import numpy as np
import pytest

import attr_ref
from conftest import pkg, random_cloud


# ------------------------------------------------------------------ the proxy
class Recorder:
    """stands in for the ctypes library: .calls holds (name, number, ...) per call, pointers left out (a ctx or an
    address passed as a plain int is a pointer by its prototype)"""

    def __init__(self, lib):
        self._lib, self._protos, self.calls = lib, pkg("_abi").PROTOTYPES, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        kinds = self._protos[name][1]

        def call(*args):
            self.calls.append((name,) + tuple(a for a, k in zip(args, kinds) if k is not C.c_void_p and type(a) in (int, float)))
            return fn(*args)
        return call


def recorded(geo, call):
    """(what `call` returned, the library calls it made)"""
    lib = geo.rt.lib
    proxy = Recorder(lib)
    geo.rt.lib = proxy
    try:
        out = call()
    finally:
        geo.rt.lib = lib
    return out, proxy.calls


# ------------------------------------------------------------------ the inputs: the smallest that reach every branch
VOXEL = 0.5


def inputs():
    """four frames: 300 rows of int32 (the corners of the range, 40 repeated rows), no row, one row, 257 rows of
    int16 (one past a workgroup of 256); the same lattice times VOXEL as float32, five NaN rows in frame 0 and frame 2
    NaN alone; uint8 x 3 attributes for both, and behind those two draws for the integer frames"""
    rng = np.random.default_rng(20)
    base = np.concatenate([random_cloud(rng, 258, extent=1000, lo=-500)[:, 1:], [[-32768] * 3, [32767] * 3]]).astype(np.int32)
    f0 = np.concatenate([base, base[:40]])[rng.permutation(300)]
    f3 = random_cloud(rng, 257)[:, 1:].astype(np.int16)
    ints = [f0, np.zeros((0, 3), np.int32), np.array([[7, -8, 9]], np.int32), f3]
    distinct = [base, ints[1], ints[2], f3]
    floats = [(f.astype(np.float32) * np.float32(VOXEL)) for f in ints]
    floats[0] = np.concatenate([floats[0][:100], np.full((5, 3), np.nan, np.float32), floats[0][100:]])
    floats[2] = np.full((1, 3), np.nan, np.float32)
    attrs = lambda frames: [rng.integers(0, 256, (f.shape[0], 3)).astype(np.uint8) for f in frames]      # noqa: E731
    return {"ints": ints, "distinct": distinct, "floats": floats, "float_attrs": attrs(floats), "distinct_attrs": attrs(distinct),
            "int_attrs": attrs(ints)}


def on_device(geo, frames):
    import torch
    return [torch.from_numpy(f).to(geo.rt.device) for f in frames]


def centres(geo, frames, k=1):
    return [(c << k) + ((1 << k) >> 1) for c in geo.decompress(geo.compress(frames), lod=k)]


# the attribute settings that reach an encode entry point of their own (max_error's is in FLOAT_KW)
ATTR_KW = [{}, dict(scalable=True), dict(cross_channel=True), dict(qstep=8), dict(qstep=(4, 8, 8), colour="ycocg"),
           dict(qstep=8, scalable_to=2), dict(qstep=(4, 8, 8), colour="ycocg", target_bytes=400)]
FLOAT_KW = dict(voxel=VOXEL, invalid="drop", lod=2, scalable=True, max_error=1, return_index=True)


def cases(geo, x):
    """name -> the call; what a call needs beside its frames is made here, outside the recording"""
    dev_ints, dev_floats = on_device(geo, x["ints"]), on_device(geo, x["floats"])
    ctr, ctr_distinct = centres(geo, x["ints"]), centres(geo, x["distinct"])
    ctr_attrs = [np.full((c.shape[0], 3), 9, np.uint8) for c in ctr_distinct]
    return {
        "integer host": lambda: geo.compress(x["ints"]),
        "integer device": lambda: geo.compress(dev_ints),
        "int16 alone": lambda: geo.compress(x["ints"][3:]),
        "float32 host": lambda: geo.compress(x["floats"], attributes=x["float_attrs"], **FLOAT_KW),
        "float32 device": lambda: geo.compress(dev_floats, attributes=x["float_attrs"], **FLOAT_KW),
        "distortion": lambda: geo.distortion(x["ints"], ctr, peak=65535),
        "distortion with attributes": lambda: geo.distortion(x["distinct"], ctr_distinct, attributes_a=x["distinct_attrs"],
                                                             attributes_b=ctr_attrs),
        **{"attributes" + (": " + ", ".join(kw) if kw else ""): lambda kw=kw: geo.compress(x["ints"], attributes=x["int_attrs"], **kw)
           for kw in ATTR_KW},
        "attributes: rows dropped": lambda: geo.compress(x["floats"], attributes=x["float_attrs"], voxel=VOXEL, invalid="drop"),
    }


# recorded on the parent commit (see the module's docstring); never taken from the tree under test
EXPECTED = {
    "integer host": [
        ("pcc_morton_keys_frames", 4, 558, 4),
        ("pcc_sort_pairs", 558, 0),
        ("pcc_keys_to_coords", 558),
        ("pcc_unique_rows", 558),
        ("pcc_gather_rows", 518, 8),
        ("pcc_octree_encode_frames", 518, 4, 0, 25190),
    ],
    "integer device": [
        ("pcc_morton_keys_frames", 4, 558, 4),
        ("pcc_sort_pairs", 558, 0),
        ("pcc_keys_to_coords", 558),
        ("pcc_unique_rows", 558),
        ("pcc_gather_rows", 518, 8),
        ("pcc_octree_encode_frames", 518, 4, 0, 25190),
    ],
    "int16 alone": [
        ("pcc_morton_keys_frames", 2, 257, 1),
        ("pcc_sort_pairs", 257, 0),
        ("pcc_keys_to_coords", 257),
        ("pcc_unique_rows", 257),
        ("pcc_octree_encode_frames", 257, 1, 0, 8465),
    ],
    "float32 host": [
        ("pcc_morton_keys_frames_f32", 563, 4, 0.5, 1),
        ("pcc_sort_pairs", 563, 0),
        ("pcc_keys_to_coords", 557),
        ("pcc_unique_rows", 557),
        ("pcc_gather_rows", 511, 8),
        ("pcc_octree_encode_frames", 511, 4, 6, 25071),
        ("pcc_attr_encode_frames_nl", 2, 4, 511, 557, 6, 1, 55628),
        ("pcc_rows_index", 563, 557, 511, 4),
    ],
    "float32 device": [
        ("pcc_morton_keys_frames_f32", 563, 4, 0.5, 1),
        ("pcc_sort_pairs", 563, 0),
        ("pcc_keys_to_coords", 557),
        ("pcc_unique_rows", 557),
        ("pcc_gather_rows", 511, 8),
        ("pcc_octree_encode_frames", 511, 4, 6, 25071),
        ("pcc_attr_encode_frames_nl", 2, 4, 511, 557, 6, 1, 55628),
        ("pcc_rows_index", 563, 557, 511, 4),
        ("pcc_sync",),
    ],
    "distortion": [
        ("pcc_morton_keys_frames", 4, 558, 4),
        ("pcc_sort_pairs", 558, 0),
        ("pcc_keys_to_coords", 558),
        ("pcc_unique_rows", 558),
        ("pcc_gather_rows", 518, 8),
        ("pcc_morton_keys_frames", 4, 517, 4),
        ("pcc_sort_pairs", 517, 0),
        ("pcc_keys_to_coords", 517),
        ("pcc_unique_rows", 517),
        ("pcc_nn_frames", 558, 517, 4),
        ("pcc_sync",),
        ("pcc_nn_frames", 517, 518, 4),
        ("pcc_sync",),
    ],
    "distortion with attributes": [
        ("pcc_morton_keys_frames", 4, 518, 4),
        ("pcc_sort_pairs", 518, 0),
        ("pcc_keys_to_coords", 518),
        ("pcc_unique_rows", 518),
        ("pcc_morton_keys_frames", 4, 517, 4),
        ("pcc_sort_pairs", 517, 0),
        ("pcc_keys_to_coords", 517),
        ("pcc_unique_rows", 517),
        ("pcc_nn_frames", 518, 517, 4),
        ("pcc_sync",),
        ("pcc_nn_frames", 517, 518, 4),
        ("pcc_sync",),
        ("pcc_gather_rows", 518, 4),
        ("pcc_gather_rows", 517, 4),
        ("pcc_nn_attr_sse_frames", 518, 517, 1, 4, 4),
        ("pcc_sync",),
        ("pcc_nn_attr_sse_frames", 517, 518, 1, 4, 4),
        ("pcc_sync",),
    ],
    "attributes: rows dropped": [
        ("pcc_morton_keys_frames_f32", 563, 4, 0.5, 1),
        ("pcc_sort_pairs", 563, 0),
        ("pcc_keys_to_coords", 557),
        ("pcc_unique_rows", 557),
        ("pcc_gather_rows", 517, 8),
        ("pcc_octree_encode_frames", 517, 4, 0, 25173),
        ("pcc_attr_encode_frames_kept", 1, 4, 517, 557, 0, 56592),
    ],
}
# the integer frames with attributes: the six calls of "integer host", then the encode entry point of the settings;
# recorded, as the lists above, on the commit before the attribute settings of a call became one record
EXPECTED.update({name: EXPECTED["integer host"] + [call] for name, call in {
    "attributes": ("pcc_attr_encode_frames", 4, 518, 56688),
    "attributes: scalable": ("pcc_attr_encode_frames_v2", 4, 518, 0, 56688),
    "attributes: cross_channel": ("pcc_attr_encode_frames_cross", 1, 4, 518, -1, 0, 0, 56688),
    "attributes: qstep": ("pcc_attr_encode_frames_transform", 4, 518, -1, 0, 8, 56688),
    "attributes: qstep, colour": ("pcc_attr_encode_frames_transform2", 4, 518, -1, 0, 1, 56688),
    "attributes: qstep, scalable_to": ("pcc_attr_encode_frames_transform3", 4, 518, -1, 0, 0, 2, 56688),
    "attributes: qstep, colour, target_bytes": ("pcc_attr_encode_frames_rate", 4, 518, -1, 0, 1, 1, 0, 56688),
}.items()})


@pytest.fixture(scope="module")
def geo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = pkg().GeometryCodec()
    yield g
    g.close()


@pytest.mark.gpu
def test_library_calls_of_a_call(geo):
    x = inputs()
    assert [f.shape[0] for f in x["ints"]] == [300, 0, 1, 257] and np.unique(x["ints"][0], axis=0).shape[0] == 260
    got, results = {}, {}
    for name, call in cases(geo, x).items():
        results[name], got[name] = recorded(geo, call)
    for name in EXPECTED:
        assert got[name] == EXPECTED[name], name
    assert set(got) == set(EXPECTED)
    # the duplicate of frame 0 asks for the gather in front of the encoder; a call without one does not
    names = [c[0] for c in got["integer host"]]
    assert names == ["pcc_morton_keys_frames", "pcc_sort_pairs", "pcc_keys_to_coords", "pcc_unique_rows", "pcc_gather_rows",
                     "pcc_octree_encode_frames"]
    assert [c[0] for c in got["int16 alone"]] == names[:4] + names[5:]
    front = names[:5]
    assert [c[0] for c in got["distortion"]] == front + front[:4] + ["pcc_nn_frames", "pcc_sync"] * 2
    # device frames give the host frames' results
    assert results["integer device"] == results["integer host"]
    h, d = results["float32 host"], results["float32 device"]
    assert d[0] == h[0] and d[1] == h[1] and all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(d[2], h[2]))


# ------------------------------------------------------------------ nothing to code
@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_nothing_to_code(geo, oracle, device):
    """no row at all, every row dropped, and an empty frame beside a coded one: the same empty blobs, the attribute
    blobs of frames without points, and an index of -1 for every input row"""
    import torch
    z, one = np.zeros((0, 3), np.int32), np.array([[1, 2, 3]], np.int32)
    nan3, nan7 = np.full((3, 3), np.nan, np.float32), np.full((7, 3), np.nan, np.float32)
    calls = [([z, z], {}), ([nan3, nan7], dict(voxel=0.5, invalid="drop")), ([z, one], {})]
    no_values = attr_ref.encode(np.zeros((0, 3), np.uint8), 1)
    empty = oracle.octree_encode(z, 32768, version=2)
    assert len(empty) == 24
    for frames, kw in calls:
        given = on_device(geo, frames) if device else frames
        coded = [f.shape[0] > 0 and not np.isnan(f).any() for f in frames]
        attrs = [np.full((f.shape[0], 3), 200, np.uint8) for f in frames]
        for with_attrs in (False, True):
            for with_index in (False, True):
                out = geo.compress(given, attributes=attrs if with_attrs else None, return_index=with_index, **kw)
                out = (out,) if not (with_attrs or with_index) else out
                assert len(out) == 1 + with_attrs + with_index
                assert all(b == empty for b, c in zip(out[0], coded) if not c) and len(out[0]) == 2
                if with_attrs:
                    assert all(b == no_values for b, c in zip(out[1], coded) if not c) and len(out[1]) == 2
                if with_index:
                    for f, idx, c in zip(frames, out[-1], coded):
                        if device:
                            assert isinstance(idx, torch.Tensor) and idx.device == geo.rt.device and idx.dtype == torch.int32
                            idx = idx.cpu().numpy()
                        assert isinstance(idx, np.ndarray) and idx.dtype == np.int32
                        assert idx.tolist() == ([0] if c else [-1] * f.shape[0])
