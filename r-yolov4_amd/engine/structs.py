"""The POD parameter blocks of csrc/conv.hip, elementwise.hip and loss.hip as ctypes classes (read from include/ryolo_params.h by abi.py,
checked against the library's own sizeof at load time) and the constants that go into them."""
import ctypes as C

from .. import abi, hip

P, I, L, F, D, Z = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_size_t
TapClass, ConvGemmParams, WgradParams, StemParams, StemWgradParams, StemBwdParams, BnActParams, PoolParams, UpParams, PackEntry, LossParams = (
    abi.STRUCTS[n] for n in ("TapClass", "ConvGemmParams", "WgradParams", "StemParams", "StemWgradParams", "StemBwdParams", "BnActParams",
                             "PoolParams", "UpParams", "PackEntry", "LossParams"))
MAX_TAPS = TapClass.dh.size                           # RY_MAX_TAPS
EPI_RAW, EPI_STATS, EPI_AFFINE_ACT, EPI_F32_BIAS, EPI_ACCUM, EPI_AFFINE_ACT_R = range(6)
ACT = {"linear": 0, "mish": 1, "leaky": 2, "swish": 3}


class KernelWord(int):
    """The kernel word of ryolo_conv_gemm_plan (ryolo.h): family in bits 0-7; generic kernel: bit 8 = its 1x1 instantiation, bits 12-15 = tile
    rows / 64; generic, patch and gemm256 kernels: bits 16-19 = tile columns / 32."""
    family = property(lambda w: w & 0xff)
    is_1x1 = property(lambda w: bool(w & 0x100))
    tile_rows = property(lambda w: ((w >> 12) & 15) * 64)
    tile_cols = property(lambda w: ((w >> 16) & 15) * 32)


_checked = False


def check_layouts():
    """Fail loudly if the library was built from other layouts than the header this process read."""
    global _checked
    if _checked:
        return
    sizes = (I * 11)()
    hip.call("ryolo_struct_sizes", sizes)
    want = [BnActParams, PoolParams, UpParams, PackEntry, ConvGemmParams, WgradParams, LossParams, TapClass, StemParams, StemWgradParams, StemBwdParams]
    for k, t in enumerate(want):
        if sizes[k] != C.sizeof(t):
            raise RuntimeError(f"ryolov4_amd: struct layout mismatch for {t.__name__}: C {sizes[k]} vs ctypes {C.sizeof(t)}")
    _checked = True
