"""Device-resident and float attributes (pcc_attr_stage_frames): the restatement of the rule (tests/attr_stage_ref.py)
on hand-worked values, the ABI, and the refusals that need no device.  No GPU;
tests/test_geometry_attributes_device_gpu.py holds the device to the restatement.
"""
import ctypes as C
import os

import numpy as np
import pytest

import attr_stage_ref as ref
from conftest import ROOT, pkg


def test_restatement_hand_worked():
    for ft in (np.float32, np.float64):
        # ties go to the even integer
        assert ref.quantise(np.array([0.5, 1.5, 2.5], ft), 1, np.uint8).tolist() == [0, 2, 2]
        # below 0, and -0.0
        assert ref.quantise(np.array([-0.0, -3.7, -0.4], ft), 1, np.uint8).tolist() == [0, 0, 0]
        # the clamp is on the float: 255.5 rounds to 256 and is cut to the peak, it does not wrap to 0
        assert ref.quantise(np.array([255.49, 255.5, 300.0, 1e30], ft), 1, np.uint8).tolist() == [255, 255, 255, 255]
        assert ref.quantise(np.array([255.5, 300.0, 65535.5, 1e30], ft), 1, np.uint16).tolist() == [256, 300, 65535, 65535]
        # a denormal times a small scale is still 0, and so is the smallest denormal times the largest scale
        tiny = np.array([np.finfo(ft).smallest_subnormal, -np.finfo(ft).smallest_subnormal], ft)
        assert ref.quantise(tiny, 1, np.uint8).tolist() == [0, 0] and ref.quantise(tiny, 65535, np.uint16).tolist() == [0, 0]
        # a product that overflows the format is clamped like any other
        assert ref.quantise(np.array([np.finfo(ft).max, -np.finfo(ft).max], ft), 65535, np.uint16).tolist() == [65535, 0]
        # k / 255 comes back as k in both precisions: the colours of a camera survive [0, 1]
        k = np.arange(256)
        assert ref.quantise((k / 255.0).astype(ft), 255, np.uint8).tolist() == k.tolist()
        assert ref.quantise((np.arange(65536) / 65535.0).astype(ft), 65535, np.uint16).tolist() == list(range(65536))
    # the arithmetic is in the source's precision: 1.5 - 1e-10 is below the tie as a double and on it as a float32
    x = np.array([1.5 - 1e-10])
    assert x.astype(np.float32)[0] == np.float32(1.5)
    assert ref.quantise(x, 1, np.uint8).tolist() == [1] and ref.quantise(x.astype(np.float32), 1, np.uint8).tolist() == [2]
    # and the scale is narrowed once: 0.3 as a float32 is 0.30000001.., so 95 * float32(0.3) is 28.500002 in float32,
    # above the tie, while the double product rounds to 28.5 itself, the tie, which goes to the even 28
    assert ref.quantise(np.array([95.0], np.float32), 0.3, np.uint8).tolist() == [29]
    assert ref.quantise(np.array([95.0], np.float64), 0.3, np.uint8).tolist() == [28]
    with pytest.raises(AssertionError):
        ref.quantise(np.array([np.nan]), 1, np.uint8)


def test_restatement_layouts():
    frames = [np.arange(15, dtype=np.uint8).reshape(5, 3), np.zeros((0, 2), np.uint16), np.array([7, 9], np.uint16)]
    out, offs = ref.packed(frames)
    assert offs == [0, 16, 16] and out.shape == (32,)
    assert out[:15].tolist() == list(range(15)) and out[15] == 0xEE      # 15 bytes in front of a pad
    assert out[16:20].view(np.uint16).tolist() == [7, 9] and (out[20:] == 0xEE).all()
    rows = ref.sorted_rows(frames, [6, 0, 9, 5], np.uint16, 4)
    assert rows.tolist() == [[9, 0, 0, 0], [0, 1, 2, 0], [0, 0, 0, 0], [7, 0, 0, 0]]
    # float frames take the destination's width in both modes
    out, offs = ref.packed([np.array([[0.5, 1.0]]), np.array([2.0], np.float32)], 1000, np.uint16)
    assert offs == [0, 16] and out[:4].view(np.uint16).tolist() == [500, 1000] and out[16:18].view(np.uint16).tolist() == [2000]


def test_stage_abi_is_declared_and_bound():
    abi = pkg("_abi")
    text = open(os.path.join(ROOT, "include", "pcc.h")).read()
    name = "pcc_attr_stage_frames"
    assert name + "(" in text and name in abi.PROTOTYPES
    res, args = abi.PROTOTYPES[name]
    vp, i64, i32, f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double
    assert res is i32 and args == [vp, vp, vp, vp, vp, i32, f64, i32, i32, vp, vp, i64, vp]
    fn = getattr(abi.lib(), name)
    assert fn.restype is i32 and list(fn.argtypes) == args
    assert abi.lib().pcc_abi_version() == 1
    for word in ("v = clamp(rint(x * s), 0, peak)", "zero-extended", "__fmul_rn", "s is not written into any blob",
                 "writes a zero row and sets status bit 1", "typedef struct pcc_attr_stage_frame"):
        assert word in text, word
    assert pkg("runtime").ATTR_SRC_KINDS == {str(k): v for k, v in ref.KINDS.items()}
    # refused without touching a device: no context
    assert fn(None, None, None, None, None, 1, 1.0, 1, 0, None, None, 0, None) != 0
    assert b"pcc_attr_stage_frames: null arrays" in abi.lib().pcc_last_error()


def test_refusals_on_the_host():
    G = pkg("geometry").GeometryCodec
    frames = [np.zeros((3, 3), np.int16)] * 2
    u8 = np.zeros((3, 3), np.uint8)
    # host integers: the arrays of before
    out = G._check_attributes(frames, [u8, u8[:, 0]])
    assert all(isinstance(a, np.ndarray) for a in out) and out[1].shape == (3, 1)
    for bad in (np.float32, np.float64):
        with pytest.raises(TypeError, match=r"^frame 1: expected uint8 or uint16 attributes, got float.*attribute_scale"):
            G._check_attributes(frames, [u8, u8.astype(bad)])
    for bad in (np.int32, np.float16, np.int8):
        with pytest.raises(TypeError, match="^frame 0: expected uint8 or uint16 attributes, got " + np.dtype(bad).name + "$"):
            G._check_attributes(frames, [u8.astype(bad), u8], None, 255.0, np.dtype(np.uint8))
    with pytest.raises(ValueError, match="frame 1: attribute_scale with uint8 attributes"):
        G._check_attributes(frames, [u8.astype(np.float32), u8], None, 255.0, np.dtype(np.uint8))
    # the scale and what float values become
    assert G._check_attribute_scale(None, None, True) == (None, None)
    assert G._check_attribute_scale(255, None, True) == (255.0, np.dtype(np.uint8))
    assert G._check_attribute_scale(255.5, None, True) == (255.5, np.dtype(np.uint16))
    assert G._check_attribute_scale(1000, np.uint8, True) == (1000.0, np.dtype(np.uint8))
    assert G._check_attribute_scale(np.float32(2), "uint16", True) == (2.0, np.dtype(np.uint16))
    for bad in (0, -1.0, 70000, float("nan"), float("inf"), 65535.5):
        with pytest.raises(ValueError, match="0 < s <= 65535"):
            G._check_attribute_scale(bad, None, True)
    for bad in (True, "255", None):
        if bad is not None:
            with pytest.raises(TypeError, match="attribute_scale must be a number"):
                G._check_attribute_scale(bad, None, True)
    with pytest.raises(ValueError, match="needs attributes"):
        G._check_attribute_scale(255, None, False)
    for bad in (np.int8, np.float32, "no such dtype"):
        with pytest.raises(ValueError, match="attribute_dtype must be np.uint8 or np.uint16"):
            G._check_attribute_scale(255, bad, True)
    with pytest.raises(ValueError, match="needs attribute_scale"):
        G._check_attribute_scale(None, np.uint8, True)
    # host float arrays become records that are staged on the device: shape, dtype and nbytes as the array they become
    (a,) = G._check_attributes(frames[:1], [np.ones((3, 2), np.float64)], None, 1000.0, np.dtype(np.uint16))
    assert not isinstance(a, np.ndarray) and a.shape == (3, 2) and a.dtype == np.uint16 and a.nbytes == 12 and not a.on_device
    assert a.kind == 3 and a.pitch == 2 and a.src.flags.c_contiguous
