"""The generic implicit-GEMM kernel (`conv_gemm_kernel`, csrc/conv.hip: kernel family 0 of `ryolo_conv_gemm`) directly through the C ABI,
BIT-EXACT against the float64 reference of tests/conv_ref.py on integer lattices (tests/conv_gemm_cases.py states the method and the
memory discipline).  Family 0 takes everything the specialised kernels decline: stride-2 forwards, small / narrow / short 1x1 layers,
3x3 layers the patch kernels refuse, the stride-2 data gradient in four output-parity classes with the class-chunked block order, the
fused MaxPool-gradient and depth-to-space stores outside the persistent kernels' ranges, and the fp32 head store.

Every case asserts through `ryolo_conv_gemm_plan` that it runs family 0 on the expected tile (and the 1x1 instantiation T1 where
expected); the test ids and docstrings name the instantiation.  Dispatch branches of `ryolo_conv_gemm` covered, by test:
  register-staged 256x32 / 128x64 / 128x128 (pipe & 0xff == 0)          test_tiles_and_mainloops[pipe0-*], test_pool_gradient, test_error_paths
  LDS-DMA 256x32                                                          test_tiles_and_mainloops[pipe1-8|24|32], test_stride2_data_gradient_classes[*-32]
  LDS-DMA 256x64 (default on >= 256 * 1536 rows)                          test_wide_tile_by_default
  deep rings 6 / 4 (by grid size; forced depths in the child)             test_ring_depth_by_grid_size
  LDS-DMA 128x64, 32- and 64-channel stages, 0x800                        test_tiles_and_mainloops[pipe1-40|64|*-0x800], test_channel_stages
  LDS-DMA 128x128, 32- and 64-channel stages                              test_tiles_and_mainloops[pipe1-72..200], test_channel_stages
  launch_gemm T1 x (accumulate, not)                                      test_pointwise_t1_and_not
  launch_gemm ID x (accumulate, not)                                      test_tiles_and_mainloops, test_forward_geometry
  launch_gemm non-ID x (accumulate, not)                                  test_stride2_data_gradient_*, test_strided_grid_rows_*, test_depth_to_space, test_pool_gradient
The knobs read once per process (RYOLO_GEMM_CLS_CHUNK, _T1, _N64, _DEEP) rerun a subset in two child processes (test_knobs_*)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, STATS, AFFINE, F32, ACCUM = 0, 1, 2, 3, 4


def _tile(Nout, pipe):
    if Nout <= 32:
        return (256, 32)
    if Nout <= 64 or ((pipe & 0xff) and (pipe & 0x800)):
        return (128, 64)
    return (128, 128)


# ------------------------------------------------------------------------------------------------ tiles and mainloops
@pytest.mark.parametrize("Nout", [8, 24, 32, 40, 64, 72, 128, 136, 200])
@pytest.mark.parametrize("pipe", [0x000, 0x001, 0x801], ids=["pipe0", "pipe1", "pipe1-0x800"])
def test_tiles_and_mainloops(pipe, Nout):
    """3x3 stride 1 with the patch kernels not asked for (no 0x200), 2 x 13 x 13 (338 rows: the last tile is partial, tiles span the image
    boundary), Cin = 32: 256x32 (Nout <= 32), 128x64 (<= 64, or 0x800 on the LDS-DMA mainloop), 128x128; register-staged and LDS-DMA
    mainloops; ID instantiations with EP 0 (raw, statistics) and EP 1 (accumulate); both lattices."""
    from tests.conv_gemm_cases import fwd
    tile = _tile(Nout, pipe)
    for epi, kind in ((RAW, "round"), (RAW, "exact"), (ACCUM, "round"), (STATS, "exact"), (STATS, "round")):
        fwd(2, 13, 13, 32, Nout, epi=epi, kind=kind, pipe=pipe, tile=tile, t1=False, seed=Nout + epi, what=f"3x3 Nout={Nout} pipe={pipe:#x} epi={epi} {kind}")


@pytest.mark.parametrize("Cin", [32, 64, 96, 128, 256, 320])
@pytest.mark.parametrize("force32", [0, 0x100], ids=["k64-if-eligible", "0x100"])
def test_channel_stages(Cin, force32):
    """9 taps on the LDS-DMA mainloop: Cin in {64, 128, 256} runs 64-channel stages (2-deep ring) unless 0x100 forces 32-channel ones;
    Cin in {32, 96, 320} never does.  Nout = 64 (128x64) and Nout = 128 with 0x800 (128x64, several column tiles) and without (128x128: from
    nk >= 12, i.e. Cin >= 64 here, the 6-deep ring takes these small grids on 32-channel stages; Cin = 32, nk = 9, runs the default ring)."""
    from tests.conv_gemm_cases import fwd
    pipe = 0x001 | force32
    for epi in (RAW, ACCUM, STATS):
        fwd(1, 9, 11, Cin, 64, epi=epi, pipe=pipe, tile=(128, 64), t1=False, seed=Cin + epi, what=f"Cin={Cin} Nout=64 pipe={pipe:#x} epi={epi}")
    fwd(1, 9, 11, Cin, 128, epi=RAW, pipe=pipe | 0x800, tile=(128, 64), seed=Cin, what=f"Cin={Cin} Nout=128 pipe={pipe | 0x800:#x}")
    fwd(1, 9, 11, Cin, 128, epi=RAW, pipe=pipe, tile=(128, 128), seed=Cin + 1, what=f"Cin={Cin} Nout=128 pipe={pipe:#x}")


def test_128x128_tile_with_64_channel_stages():
    """More than 512 tiles (5 x 116 x 116 = 67 280 rows -> 526): past the deep rings, so Cin = 64 / 9 taps runs the 128x128 tile on
    64-channel stages (raw and accumulate instantiations), and with 0x100 on the default 3-stage ring."""
    from tests.conv_gemm_cases import fwd
    fwd(5, 116, 116, 64, 128, epi=RAW, pipe=0x001, tile=(128, 128), seed=1, what="128x128 KB=64")
    fwd(5, 116, 116, 64, 128, epi=ACCUM, pipe=0x001, tile=(128, 128), seed=3, what="128x128 KB=64 accumulate")
    fwd(5, 116, 116, 64, 128, epi=ACCUM, pipe=0x101, tile=(128, 128), seed=2, what="128x128 KB=32 ring 3")


def test_long_reduction():
    """K = 9 x 512 (144 steps) on the three tiles, both mainloops; the shortest K (one step: one tap, 32 channels) is in test_pointwise_t1_and_not."""
    from tests.conv_gemm_cases import fwd
    for Nout, pipe in ((32, 0x001), (64, 0x001), (136, 0x001), (136, 0x000), (32, 0x000)):
        fwd(2, 7, 9, 512, Nout, epi=RAW, pipe=pipe, tile=_tile(Nout, pipe), seed=Nout, what=f"K=4608 Nout={Nout} pipe={pipe:#x}")
    fwd(2, 7, 9, 512, 136, epi=STATS, kind="exact", pipe=0x001, tile=(128, 128), seed=3, what="K=4608 exact statistics")


@pytest.mark.parametrize("epi", [RAW, ACCUM, STATS])
def test_pointwise_t1_and_not(epi):
    """1x1 layers.  T1 (the 1x1 instantiation: LDS-DMA mainloop, identity grid, tap (0, 0), weight slot 0) with ldA > Cin and K from one
    step up; NOT T1: the register-staged mainloop, a 1x1 stride-2 layer, a single tap with widx != 0, a single shifted tap."""
    from tests.conv_gemm_cases import fwd, run_lattice
    for Cin, Nout in ((32, 8), (32, 64), (64, 136), (96, 40), (320, 200)):
        fwd(3, 11, 7, Cin, Nout, k=1, epi=epi, pipe=0x001, ldA_extra=24, tile=_tile(Nout, 1), t1=True, seed=Cin + Nout, what=f"T1 {Cin}->{Nout} epi={epi}")
        fwd(3, 11, 7, Cin, Nout, k=1, epi=epi, pipe=0x000, tile=_tile(Nout, 0), t1=False, seed=Cin + Nout, what=f"1x1 register-staged {Cin}->{Nout} epi={epi}")
    fwd(2, 13, 9, 64, 72, k=1, s=2, epi=epi, pipe=0x001, tile=(128, 128), t1=False, seed=5, what=f"1x1 stride 2 epi={epi}")
    fwd(2, 26, 14, 32, 24, k=1, s=2, epi=epi, pipe=0x001, tile=(256, 32), t1=False, seed=6, what=f"1x1 stride 2 Nout=24 epi={epi}")
    for taps in ([(0, 0, 2)], [(1, -1, 0)]):
        run_lattice(NB=2, IH=9, IW=10, Cin=64, Nout=40, wtaps=3, OH=9, OW=10, classes=[(taps, 0, 0)], epi=epi, pipe=0x001, tile=(128, 64),
                    t1=False, seed=7, what=f"single tap {taps} epi={epi}")


@pytest.mark.parametrize("geom,stages", [((3, 65, 65), 6), ((3, 92, 92), 4), ((3, 113, 113), 3)], ids=["200-tiles-6", "398-tiles-4", "600-tiles-default"])
def test_ring_depth_by_grid_size(geom, stages):
    """Nout = 136 (two column tiles), 1x1 with Cin = 384 (nk = 12: the threshold) -> <= 256 tiles run the 6-deep ring, 257-512 the 4-deep one,
    more the default; Cin = 352 (nk = 11) stays on the default ring at every size.  T1 and (3x3, nk = 18) non-T1 instantiations, EP 0 and 1."""
    from tests.conv_gemm_cases import fwd
    for Cin in (384, 352):
        for epi in (RAW, ACCUM):
            fwd(*geom, Cin, 136, k=1, epi=epi, pipe=0x001, tile=(128, 128), t1=True, seed=Cin + epi, what=f"ring {stages} Cin={Cin} epi={epi}")
    fwd(*geom, 384, 136, k=1, epi=STATS, kind="exact", pipe=0x001, tile=(128, 128), t1=True, seed=9, what=f"ring {stages} statistics")
    if stages == 6:
        fwd(1, 40, 40, 64, 136, epi=STATS, pipe=0x101, tile=(128, 128), t1=False, seed=10, what="ring 6 non-T1 3x3 statistics")
        fwd(1, 40, 40, 64, 136, epi=ACCUM, pipe=0x101, tile=(128, 128), t1=False, seed=11, what="ring 6 non-T1 3x3 accumulate")


def test_wide_tile_by_default():
    """>= 256 * 1536 rows at Cin = 32, Nout = 64: the 256x64 tile without any knob (6 x 256 x 256 = 393 216 rows exactly, 1536 tiles).  The
    row count is the dispatch threshold itself, so the case cannot be smaller."""
    from tests.conv_gemm_cases import fwd
    fwd(6, 256, 256, 32, 64, k=1, epi=RAW, pipe=0x001, tile=(256, 64), t1=True, seed=1, what="256x64 T1")
    fwd(6, 256, 256, 32, 64, k=1, s=1, epi=ACCUM, pipe=0x001, tile=(256, 64), t1=True, seed=2, what="256x64 T1 accumulate")


# ------------------------------------------------------------------------------------------------ forward geometry
@pytest.mark.parametrize("NB", [1, 5])
@pytest.mark.parametrize("H,W", [(13, 13), (25, 25), (26, 26), (7, 9)])
def test_forward_geometry_stride2(NB, H, W):
    """3x3 stride 2 pad 1, odd and even maps (the last tap column / row exists only on even sizes)."""
    from tests.conv_gemm_cases import fwd
    for Cin, Nout, pipe in ((64, 128, 0x001), (64, 32, 0x001), (96, 64, 0x000), (128, 40, 0x001)):
        for epi in (RAW, STATS, ACCUM):
            fwd(NB, H, W, Cin, Nout, s=2, epi=epi, pipe=pipe, tile=_tile(Nout, pipe), t1=False, seed=H + epi, what=f"s2 {NB}x{H}x{W} {Cin}->{Nout} epi={epi}")


@pytest.mark.parametrize("NB", [1, 5])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (7, 9), (25, 19)])
def test_forward_geometry_stride1(NB, H, W):
    """3x3 stride 1 on the generic kernel (no 0x200): maps where every pixel is a border pixel, tiles that span image boundaries."""
    from tests.conv_gemm_cases import fwd
    for Cin, Nout, pipe in ((64, 128, 0x001), (32, 32, 0x001), (96, 64, 0x000), (64, 8, 0x000)):
        for epi in (RAW, ACCUM):
            fwd(NB, H, W, Cin, Nout, epi=epi, pipe=pipe, tile=_tile(Nout, pipe), t1=False, seed=W + epi, what=f"s1 {NB}x{H}x{W} {Cin}->{Nout} epi={epi}")


@pytest.mark.parametrize("act", [0, 1, 2, 3], ids=["linear", "mish", "leaky", "silu"])
def test_affine_act_epilogue(act):
    """EPI_AFFINE_ACT: exact accumulator, so the only error is the epilogue's own formula — one bf16 ulp + the fp32 evaluation bound of
    ew_ref.bn_act_fwd, >= 99 % bit-identical; the linear activation with power-of-two scale and lattice shift is bit-identical."""
    from tests.conv_gemm_cases import Tally, fwd
    t = Tally()
    for Cin, Nout, k, pipe in ((32, 128, 3, 0x001), (64, 40, 3, 0x001), (96, 24, 3, 0x000), (64, 136, 1, 0x001), (128, 64, 1, 0x000)):
        fwd(3, 25, 19, Cin, Nout, k=k, epi=AFFINE, act=act, pipe=pipe, tile=_tile(Nout, pipe), seed=Cin + act, tally=t, what=f"act={act} {Cin}->{Nout} k={k}")
    t.check(f"act={act}")


# ------------------------------------------------------------------------------------------------ stride-2 data gradient in four classes
@pytest.mark.parametrize("Nout", [32, 128])
@pytest.mark.parametrize("NB,OH,OW", [(1, 1, 1), (3, 3, 5), (1, 13, 13), (3, 25, 19), (1, 9, 3), (3, 40, 7), (1, 30, 25), (3, 11, 49), (1, 7, 200)])
def test_stride2_data_gradient_classes(NB, OH, OW, Nout):
    """1 / 2 / 2 / 4 live taps, oh_mul = ow_mul = 2: every pixel of the full grid written exactly once (sentinel prefill for raw, old +
    contribution for accumulate).  Single-tile maps (tiles that wrap over all images from column 0) and several tiles starting inside image rows;
    the tiles that start at the last column are in test_stride2_data_gradient_tile_at_last_column."""
    from tests.conv_gemm_cases import dgrad_s2
    for epi in (RAW, ACCUM):
        for pipe in (0x001, 0x000):
            dgrad_s2(NB, OH, OW, 64, Nout, epi=epi, pipe=pipe, tile=_tile(Nout, pipe), t1=False, seed=OW + epi, what=f"dgrad {NB}x{OH}x{OW} Nout={Nout} epi={epi} pipe={pipe}")


@pytest.mark.parametrize("Nout", [32, 128])
@pytest.mark.parametrize("NB,OH,OW", [(9, 20, 3), (7, 27, 7), (3, 14, 25), (3, 70, 49), (3, 100, 100), (1, 10, 200)])
def test_stride2_data_gradient_tile_at_last_column(NB, OH, OW, Nout):
    """OW = 3, 7, 25, 49, 100, 200 with NB x OH chosen so that a tile's first row sits at the last column a tile can reach: tile k starts at
    column k * tile_rows mod OW, a multiple of gcd(tile_rows, OW) — OW - 1 for the odd widths (256-row tiles: k = 2, 5, 4, 40; 128-row tiles:
    k = 1, 3, 8, 31); for even OW the last column is unreachable by arithmetic and the case reaches OW - gcd (96 of 100, 192 of 200).  From
    there out_pixel()'s small_div sees e_ow + rt up to OW - 1 + 255 (Nout = 32: the 256-row tile walks furthest) and the tile wraps over up to
    five image boundaries (images of 60 ... 10 000 rows).  The runner proves the tile exists from (M, OW, tile rows of the plan): edge_col."""
    from tests.conv_gemm_cases import dgrad_s2
    for epi in (RAW, ACCUM):
        for pipe in (0x001, 0x000):
            dgrad_s2(NB, OH, OW, 32, Nout, epi=epi, pipe=pipe, tile=_tile(Nout, pipe), t1=False, edge_col=True, seed=OW + epi,
                     what=f"dgrad last column {NB}x{OH}x{OW} Nout={Nout} epi={epi} pipe={pipe}")


@pytest.mark.parametrize("only", [(0,), (3,), (1, 2), (0, 1, 3)], ids=["class0", "class3", "classes12", "classes013"])
def test_strided_grid_rows_no_class_owns_stay_unchanged(only):
    """A launch with a subset of the parity classes (oh_mul = ow_mul = 2): the pixels of the other parities — whole rows of the full grid when both
    classes of a row parity are missing — belong to nobody and must come back bit for bit (sentinel for raw, the old lattice values for accumulate
    and the fp32 store), while the owned pixels equal the reference."""
    from tests.conv_gemm_cases import dgrad_s2
    for Nout in (32, 128):
        for epi in (RAW, ACCUM, F32):
            for pipe in (0x001, 0x000):
                dgrad_s2(3, 25, 19, 64, Nout, only=only, epi=epi, pipe=pipe, tile=_tile(Nout, pipe), t1=False, seed=sum(only) + epi,
                         what=f"classes {only} Nout={Nout} epi={epi} pipe={pipe}")


def test_stride2_data_gradient_last_chunk():
    """3 x 300 x 300 dY pixels at Nout = 32: 1055 tiles per class, so the class-chunked order runs one full chunk of 1024 and a last one of
    31 (nin = min(CH, T - base)).  The size is what the default chunk length demands; the child processes run short chunks on small grids."""
    from tests.conv_gemm_cases import dgrad_s2
    dgrad_s2(3, 300, 300, 32, 32, epi=RAW, pipe=0x001, tile=(256, 32), edge_col=True, seed=1, what="dgrad 1055 tiles per class")


# ------------------------------------------------------------------------------------------------ fused stores on the non-ID path
@pytest.mark.parametrize("epi", [RAW, ACCUM])
@pytest.mark.parametrize("Cin,pipe", [(32, 0x001), (512, 0x001), (128, 0x000), (64, 0x000)])
def test_pool_gradient(Cin, pipe, epi):
    """Fused MaxPool2d(2, 2) gradient on family 0 (the persistent 1x1 kernel claims Cin 64 ... 256 on the LDS-DMA mainloop only): odd image
    counts, Nout not a multiple of the tile, ld > C; one rounding after adding dz, then the accumulate step."""
    from tests.conv_gemm_cases import fwd
    for NB, H, W, Nout in ((3, 10, 14, 136), (1, 6, 6, 24), (5, 20, 20, 64), (3, 8, 4, 200)):
        fwd(NB, H, W, Cin, Nout, k=1, epi=epi, pipe=pipe, pool=True, tile=_tile(Nout, pipe), t1=False, seed=Cin + H, what=f"pool {NB}x{H}x{W} {Cin}->{Nout} pipe={pipe}")


@pytest.mark.parametrize("epi", [RAW, ACCUM])
@pytest.mark.parametrize("cin", [8, 16, 64])
def test_depth_to_space(cin, epi):
    """Space-to-depth data gradient on family 0 (families 2 and 6 claim s2d_cin == 32 only): Nout = 4 * cin = 32 / 64 / 256 columns."""
    from tests.conv_gemm_cases import s2d
    for NB, OH, OW, Cout in ((3, 25, 19, 64), (1, 7, 5, 32), (5, 16, 48, 96), (1, 1, 1, 64)):
        for pipe in (0x001, 0x000):
            s2d(NB, OH, OW, Cout, cin, epi=epi, pipe=pipe, tile=_tile(4 * cin, pipe), t1=False, seed=cin + OW, what=f"s2d {NB}x{OH}x{OW} cin={cin} pipe={pipe}")


# ------------------------------------------------------------------------------------------------ the fp32 row-major store
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("Nout", [7, 21, 54, 396])
def test_f32_bias_store(Nout, bias):
    """EPI_F32_BIAS row-major: the 16-byte store branch (ldC % 4 == 0) and the scalar one, ragged Nout, identity grid (T1 and 3x3) and the
    four-class grid of a stride-2 data gradient."""
    from tests.conv_gemm_cases import dgrad_s2, fwd
    for extra in ((-Nout) % 4 + 4, (-Nout) % 4 + 5):                         # ldC = Nout + extra: a multiple of 4, then not
        fwd(3, 11, 13, 64, Nout, k=1, epi=F32, bias=bias, pipe=0x001, ldC_extra=extra, tile=_tile(Nout, 1), t1=True, seed=Nout, what=f"f32 T1 Nout={Nout} ldC+{extra}")
        fwd(3, 11, 13, 32, Nout, k=3, epi=F32, bias=bias, pipe=0x000, ldC_extra=extra, tile=_tile(Nout, 0), seed=Nout + 1, what=f"f32 3x3 Nout={Nout} ldC+{extra}")
        dgrad_s2(2, 7, 9, 64, Nout, epi=F32, bias=bias, pipe=0x001, ldC_extra=extra, tile=_tile(Nout, 1), seed=Nout + 2, what=f"f32 classes Nout={Nout} ldC+{extra}")


# ------------------------------------------------------------------------------------------------ error paths
def test_error_paths_launch_nothing():
    """Arguments the entry point must refuse with a status, leaving the output untouched."""
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    from tests.conv_ref import taps_forward
    hip.lib()
    dev = "cuda:0"
    NB, H, W, Cin, Nout = 2, 8, 8, 64, 32
    x = torch.ones(NB * H * W + 8, Cin + 8, dtype=torch.bfloat16, device=dev)
    w = torch.ones(Nout, 9, Cin, dtype=torch.bfloat16, device=dev)
    out = torch.full((4 * NB * H * W, Nout), 5.0, dtype=torch.bfloat16, device=dev)
    stats = torch.full((64, 2, Nout), 5.0, device=dev)
    pidx = torch.zeros(NB * H * W, Nout, dtype=torch.uint8, device=dev)
    zeros = torch.zeros(256, dtype=torch.uint8, device=dev)

    def params():
        p = S.ConvGemmParams()
        p.A, p.NB, p.IH, p.IW, p.Cin, p.ldA = x.data_ptr(), NB, H, W, Cin, Cin + 8
        p.W, p.Nout, p.wtaps = w.data_ptr(), Nout, 9
        p.OH, p.OW, p.sh, p.sw = H, W, 1, 1
        p.oh_mul, p.ow_mul, p.OHf, p.OWf = 1, 1, H, W
        p.nclasses = 1
        for c in range(4):
            tc = p.cls[c]
            tc.ntaps = 9
            for t, (dh, dw, wi) in enumerate(taps_forward(3, 1)):
                tc.dh[t], tc.dw[t], tc.widx[t] = dh, dw, wi
        p.epi, p.out, p.ldC, p.stats = 0, out.data_ptr(), Nout, stats.data_ptr()
        p.zeros, p.pipe = zeros.data_ptr(), 0x001
        return p

    def refused(change, what):
        p = params()
        change(p)
        rc = hip.lib().ryolo_conv_gemm(p, hip.stream())
        torch.cuda.synchronize()
        assert rc != 0, f"{what}: accepted"
        assert bool((out == 5.0).all()) and bool((stats == 5.0).all()), f"{what}: refused with status {rc} but wrote"

    p = params()
    assert hip.lib().ryolo_conv_gemm(p, hip.stream()) == 0                      # the unmodified block is valid ...
    torch.cuda.synchronize()
    assert bool((out[:NB * H * W] == 9.0 * Cin).sum() > 0)                       # ... and launches (interior pixels: 9 taps x 64 ones = 576)
    out.fill_(5.0)
    refused(lambda p: setattr(p, "Cin", 48), "Cin % 32 != 0")
    refused(lambda p: setattr(p, "ldA", Cin + 4), "ldA % 8 != 0")
    refused(lambda p: setattr(p, "A", x.data_ptr() + 8), "A not 16-byte aligned")
    refused(lambda p: setattr(p, "W", w.data_ptr() + 2), "W not 16-byte aligned")
    refused(lambda p: setattr(p, "nclasses", 0), "nclasses = 0")
    refused(lambda p: setattr(p, "nclasses", 5), "nclasses = 5")
    refused(lambda p: setattr(p.cls[0], "ntaps", 0), "ntaps = 0")
    refused(lambda p: setattr(p.cls[0], "ntaps", 10), "ntaps = 10")

    def two_class_stats(p):
        p.nclasses, p.epi = 2, S.EPI_STATS
    refused(two_class_stats, "statistics with two classes")

    def pool_odd(p):
        p.IH = p.OH = p.OHf = 7
        p.pool_idx, p.pool_dz, p.pool_ldi, p.pool_ld = pidx.data_ptr(), out.data_ptr(), Nout, Nout
    refused(pool_odd, "pool gradient with odd OH")


# ------------------------------------------------------------------------------------------------ process-wide knobs
def _child(env, timeout=900):
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    env = dict(os.environ, RYOLO_CONV_GEMM_CHILD="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/conv_gemm_cases.py", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout


def test_knobs_classes_on_grid_z_no_t1_wide_n64_ring4():
    """RYOLO_GEMM_CLS_CHUNK=0 (classes on blockIdx.z), RYOLO_GEMM_T1=0 (1x1 layers through the tap-table instantiations), RYOLO_GEMM_N64=2
    (256x64 tiles on every grid), RYOLO_GEMM_DEEP=4 (4-deep ring on every eligible launch, nk below the ring depth included): the four knobs
    claim different launches, so they share one child."""
    _child({"RYOLO_GEMM_CLS_CHUNK": "0", "RYOLO_GEMM_T1": "0", "RYOLO_GEMM_N64": "2", "RYOLO_GEMM_DEEP": "4"})


def test_knobs_short_class_chunks_ring6():
    """RYOLO_GEMM_CLS_CHUNK=16 (many short chunks, the last one shorter) and RYOLO_GEMM_DEEP=6."""
    _child({"RYOLO_GEMM_CLS_CHUNK": "16", "RYOLO_GEMM_DEEP": "6"})
