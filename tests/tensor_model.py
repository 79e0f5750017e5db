"""The numpy model of the tensor extension (include/mpcvr.h: mpcvr_tensor_pass, mpcvr_plan_tensor_value): a surface of 32-bit RGB texels
as a float tensor.  numpy does the two fp32 roundings (a float32 multiply, then a float32 add: numpy never fuses them), astype(float16)
rounds to nearest even with overflow to inf and subnormals kept, bf16 is the header's integer formula.  Everything is bits, so the kernel
and the host function are held to it word for word."""
import numpy as np

BGRA8, RGB10A2 = 0, 1
F32, F16, BF16 = 0, 1, 2
PLANAR, INTERLEAVED = 0, 1
RGB, BGR = 0, 1
ELEMENT_SIZE = {F32: 4, F16: 2, BF16: 2}
ELEMENT_DTYPE = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}


def codes(words, src_fmt):
    """(h, w) uint32 texels -> (3, h, w) uint32 codes of R, G, B; the A / X bits are ignored"""
    t = np.asarray(words, dtype=np.uint32)
    if src_fmt == RGB10A2:
        return np.stack([t & 0x3ff, (t >> 10) & 0x3ff, (t >> 20) & 0x3ff])
    return np.stack([(t >> 16) & 0xff, (t >> 8) & 0xff, t & 0xff])


def element_bits(code, scale, bias, dtype):
    """the stored bits (uint32 / uint16 array) of code * scale + bias, elementwise; scale and bias are rounded to fp32 first, as the C struct holds them"""
    c = np.asarray(code).astype(np.float32)                     # exact: codes stay below 2^24
    with np.errstate(over="ignore"):
        t = c * np.float32(scale)                               # rounded to fp32
        v = (t + np.float32(bias)).astype(np.float32)           # rounded to fp32
        assert t.dtype == np.float32
        if dtype == F32:
            return v.view(np.uint32)
        if dtype == F16:
            return v.astype(np.float16).view(np.uint16)
    u = v.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def tensor(words, src_fmt, dtype, layout, channel_order, scale, bias):
    """(h, w) uint32 texels -> the tensor's elements as bits: (3, h, w) for PLANAR, (h, w, 3) for INTERLEAVED.  scale / bias: three each, for
    R, G, B of the picture whatever the channel order"""
    c = codes(words, src_fmt)
    planes = [element_bits(c[k], scale[k], bias[k], dtype) for k in range(3)]
    if channel_order == BGR:
        planes = planes[::-1]
    out = np.stack(planes)
    return out if layout == PLANAR else np.ascontiguousarray(out.transpose(1, 2, 0))


def place(buf, offset, bits, layout, row_pitch, plane_pitch=0):
    """writes the tensor's elements into the uint8 array `buf` at byte `offset` with the given pitches (what the pass must leave of a
    patterned buffer: these bytes changed, every other byte untouched)"""
    es = bits.dtype.itemsize
    if layout == PLANAR:
        _, h, w = bits.shape
        for k in range(3):
            for y in range(h):
                at = offset + k * plane_pitch + y * row_pitch
                buf[at:at + w * es] = bits[k, y].view(np.uint8)
    else:
        h, w, _ = bits.shape
        for y in range(h):
            at = offset + y * row_pitch
            buf[at:at + 3 * w * es] = bits[y].reshape(-1).view(np.uint8)
    return buf
