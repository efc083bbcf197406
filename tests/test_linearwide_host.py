"""Host side of the wide 1x1 operators (no GPU): the chunk rule, the workspace and the template instantiations as tests/linearwide_ref.py
restates them against the library's own entries and words, the new entries in the header, the bindings and the library, and what the
case lists of tests/test_gpu_linearwide.py reach."""
import ctypes
import os
import re

from tests import linearwide_ref as ref

ENTRIES = ('yr_linear_wide_forward', 'yr_linear_wide_dgrad', 'yr_linear_wide_wgrad_chunk', 'yr_linear_wide_wgrad_workspace_bytes',
           'yr_linear_wide_wgrad')


def _csrc(name):
    from yoloret_amd import build
    return open(os.path.join(os.path.dirname(build.__file__), 'csrc', name)).read()


def test_entries_are_in_the_header_the_bindings_and_the_library_under_abi_9():
    from yoloret_amd import build, runtime
    L = ctypes.CDLL(build.LIB)
    L.yr_abi_version.restype = ctypes.c_int
    assert L.yr_abi_version() == 9 == runtime.ABI_VERSION
    header = open(os.path.join(os.path.dirname(build.__file__), '..', 'include', 'yoloret_hip.h')).read()
    assert re.search(r'#define YR_ABI_VERSION 9\b', header)
    for sym in ENTRIES:
        getattr(L, sym)
        assert sym in runtime.EXPORTS
        assert re.search(r'\b%s\s*\(' % sym, header), sym
    assert 'linearwide.hip' in build.SOURCES
    # the narrow twins are still there, with their own cap
    for sym in ('yr_linear_forward', 'yr_linear_dgrad', 'yr_linear_wgrad'):
        getattr(L, sym)
    assert 'cin <= 256 && cout >= 1 && cout <= 256' in _csrc('headtrain.hip')
    # the twins take the same arguments
    lib = runtime.lib()
    for wide, narrow in (('yr_linear_wide_forward', 'yr_linear_forward'), ('yr_linear_wide_dgrad', 'yr_linear_dgrad'),
                         ('yr_linear_wide_wgrad', 'yr_linear_wgrad'), ('yr_linear_wide_wgrad_chunk', 'yr_linear_wgrad_chunk'),
                         ('yr_linear_wide_wgrad_workspace_bytes', 'yr_linear_wgrad_workspace_bytes')):
        assert list(getattr(lib, wide).argtypes) == list(getattr(lib, narrow).argtypes)
    assert lib.yr_linear_wide_wgrad_workspace_bytes.restype is ctypes.c_size_t


GRID_CHANNELS = (1, 3, 4, 5, 75, 128, 216, 255, 256, 257, 331, 512, 513, 576, 1021, 1023, 1024)
GRID_PIXELS = (1, 5, 64, 65, 1000, 10816, 65536, 65537, 43264, 173056, 10 ** 7, 2 ** 40 - 1)


def test_chunk_and_workspace_follow_the_restated_rule():
    from yoloret_amd import runtime as rt
    for cin in GRID_CHANNELS:
        for cout in GRID_CHANNELS:
            for pixels in GRID_PIXELS:
                c = rt.linear_wide_wgrad_chunk(pixels, cin, cout)
                assert c == ref.chunk(pixels, cin, cout), (pixels, cin, cout)
                assert c >= ref.MIN_CHUNK and c % ref.CHUNK_STEP == 0
                if ref.narrow(cin, cout):      # the narrow entry's own rule: the call is yr_linear_wgrad
                    assert c == rt.linear_wgrad_chunk(pixels, cin, cout) and -(-pixels // c) <= ref.NARROW_MAX_CHUNKS
                    assert rt.linear_wide_wgrad_workspace_bytes(pixels, cin, cout) == rt.linear_wgrad_workspace_bytes(pixels, cin, cout)
                else:
                    assert -(-pixels // c) <= ref.MAX_CHUNKS
                assert c * (cin + cout) >= cout * ref.kp_of(cin), 'a slab larger than its chunk\'s operands'
                assert rt.linear_wide_wgrad_workspace_bytes(pixels, cin, cout) == ref.workspace_bytes(pixels, cin, cout) == -(-pixels // c) * cout * ref.kp_of(cin) * 4
    for bad in ((0, 75, 75), (-1, 75, 75), (1 << 40, 75, 75), (100, 0, 75), (100, 1025, 75), (100, 75, 0), (100, 75, 1025), (100, -3, 5)):
        assert rt.linear_wide_wgrad_chunk(*bad) == 0 == ref.chunk(*bad) and rt.linear_wide_wgrad_workspace_bytes(*bad) == 0 == ref.workspace_bytes(*bad)
    # hand-derived: td1_conv of MobileNetV2 x0.75 at 64 images of 416 (13 x 13 maps): 512 * 216 / 728 = 151.9 -> 160 pixels, 68 slabs
    assert ref.chunk(64 * 169, 216, 512) == 160 and ref.workspace_bytes(64 * 169, 216, 512) == 68 * 512 * 216 * 4
    # td3_conv of MobileNetV2 x1.4 (272 -> 128, 52 x 52 maps): 173056 / 1024 = 169 -> 176 pixels, 984 slabs of 128 x 272; x0.75's 248 -> 128
    # is narrow on both sides: the narrow rule's 512 pixels, 338 slabs
    assert ref.chunk(64 * 2704, 272, 128) == 176 and ref.workspace_bytes(64 * 2704, 272, 128) == 984 * 128 * 272 * 4
    assert ref.chunk(64 * 2704, 248, 128) == 512 and ref.workspace_bytes(64 * 2704, 248, 128) == 338 * 128 * 248 * 4
    assert ref.chunk(2 ** 40 - 1, 257, 1) == 2 ** 30 < 2 ** 31 and ref.chunk(2 ** 40 - 1, 1, 1) == 2 ** 29      # the largest chunk is an int
    assert ref.chunk(1, 1024, 1024) == 512 == ref.min_chunk(1024, 1024) and ref.min_chunk(3, 257) == 64
    # narrow on both sides: headtrain.hip's rule (256 pixels, 512 past five tiles a side, 2048 slabs)
    assert ref.chunk(64 * 2704, 75, 128) == 512 and ref.chunk(64 * 2704, 75, 75) == 256
    assert ref.chunk(524289, 5, 3) == 272 and ref.chunk(2048 * 512 + 1, 255, 255) == 528 and ref.chunk(100, 256, 256) == 512 and ref.chunk(100, 257, 256) == 144


def test_the_restatement_uses_the_source_s_constants():
    src = _csrc('linearwide.hip')
    assert '#include "train_common.h"' in src
    for name, value in (('LW_MAX_C', ref.MAX_C), ('LW_MIN_CHUNK', ref.MIN_CHUNK), ('LW_MAX_CHUNKS', ref.MAX_CHUNKS), ('LW_CHUNK_STEP', ref.CHUNK_STEP),
                        ('LW_WG_TILES', ref.PRODUCT_TILES), ('LW_GW_TILES', ref.WGRAD_TILES)):
        assert re.search(r'#define %s %d\b' % (name, value), src), name
    assert 'atomic' not in src.split('#include')[1]
    from yoloret_amd import build
    flags = build.FLAGS
    assert '-ffp-contract=off' in flags


def test_kernels_use_no_scratch_and_every_instantiation_is_built():
    from yoloret_amd import build
    rows = build.kernel_resources()['linearwide.hip']
    names = [r[0] for r in rows]
    assert len(rows) == 8 + 12      # the gradient's stage 1 runs with a side above 256: TA or TB is 3 or 4
    assert all(scratch == 0 for _, _, scratch, _, _ in rows)
    for wt in range(1, 5):
        for nat in (0, 1):
            assert any('lw_product_kernelILi%dELb%dE' % (wt, nat) in n for n in names)
    for ta in range(1, 5):
        for tb in range(1, 5):
            assert any('lw_wgrad_partial_kernelILi%dELi%dE' % (ta, tb) in n for n in names) == (max(ta, tb) >= 3)
    # 4 pixel tiles x 4 channel tiles of accumulators (64 registers) and the operands fit without scratch: the widest forms
    # hold at least two waves per SIMD
    for r in rows:
        if 'lw_product_kernelILi4E' in r[0] or 'lw_wgrad_partial_kernelILi4ELi4E' in r[0]:
            assert r[3] >= 2, r


def test_gpu_cases_reach_every_instantiation():
    shapes = ref.EXACT_SHAPES
    assert {ref.product_form(cout) for _, cout in shapes} == {1, 2, 3, 4}      # the forward
    assert {ref.product_form(cin) for cin, _ in shapes} == {1, 2, 3, 4}        # the input gradient
    assert {ref.wgrad_form(cin, cout) for cin, cout in shapes if not ref.narrow(cin, cout)} == {(a, b) for a in range(1, 5) for b in range(1, 5) if max(a, b) >= 3}
    assert len(shapes) == len(set(shapes)) and sum(1 for s in shapes if ref.narrow(*s)) >= 5 and ref.wgrad_form(75, 75) is None
    # no shape with a side above 256 runs a form with both counts below 3
    assert all(max(ref.wgrad_form(a, b)) >= 3 for a in (1, 33, 128, 256, 257, 300, 400, 512, 1024) for b in (257, 288, 289, 385, 400, 513, 900, 1024))
    # hand-derived forms: 512 channels are two blocks of 16 tiles (two passes), 256 one; 257 is 17 tiles = two blocks of 9
    assert ref.blocking(512, 16) == (2, 16) and ref.blocking(256, 16) == (1, 16) and ref.blocking(257, 16) == (2, 9) and ref.blocking(1024, 16) == (4, 16)
    assert ref.product_form(512) == 4 and ref.product_form(257) == 3 and ref.product_form(75) == 2 and ref.product_form(3) == 1
    assert ref.blocking(257, 8) == (3, 6) and ref.blocking(216, 8) == (2, 7) and ref.wgrad_form(216, 512) == (4, 4) and ref.wgrad_form(257, 3) == (1, 3)
    assert ref.kernel_names(216, 512) == ('lw_product_kernel<4,0>', 'lw_product_kernel<4,1>', 'lw_wgrad_partial_kernel<4,4>')
    # the issue's shapes are all there
    for s in [(216, 512), (512, 75), (424, 256), (331, 512), (272, 128), (576, 256), (512, 255), (257, 3), (3, 257), (257, 257), (1021, 513),
              (1024, 1024), (75, 75), (248, 128)]:
        assert s in shapes
    assert ref.PIXELS == [1, 5, 63, 64, 65]


def test_gpu_cases_have_ragged_last_blocks_on_either_side():
    shapes = ref.EXACT_SHAPES
    # a last tile that is not full, on either side, in all three entries
    assert any(cin % 16 and not cout % 16 for cin, cout in shapes) and any(cout % 16 and not cin % 16 for cin, cout in shapes)
    assert any(cin % 16 and cout % 16 for cin, cout in shapes)
    # a last block with a whole tile past the channel count: on the output side of the forward (cout) and of the input gradient
    # (cin), on either side and on both sides of the weight gradient
    assert ref.idle_tiles(257, ref.PRODUCT_TILES) == 1 and ref.idle_tiles(257, ref.WGRAD_TILES) == 1 and ref.idle_tiles(513, ref.PRODUCT_TILES) == 0
    assert any(ref.idle_tiles(cout, ref.PRODUCT_TILES) for _, cout in shapes) and any(ref.idle_tiles(cin, ref.PRODUCT_TILES) for cin, _ in shapes)
    idle = [(bool(ref.idle_tiles(cin, ref.WGRAD_TILES)), bool(ref.idle_tiles(cout, ref.WGRAD_TILES))) for cin, cout in shapes if not ref.narrow(cin, cout)]
    assert (True, False) in idle and (False, True) in idle and (True, True) in idle
    # a wave without any tile (fewer tiles than waves) and a wave with a tile less than its neighbours
    assert any(ref.blocking(cout, ref.PRODUCT_TILES)[1] < 4 for _, cout in shapes)
    assert any(ref.blocking(cout, ref.PRODUCT_TILES)[1] % 4 for _, cout in shapes if cout > 256)
    assert any(ref.blocking(cout, ref.WGRAD_TILES)[1] == 1 for _, cout in shapes) and any(ref.blocking(cin, ref.WGRAD_TILES)[1] % 2 for cin, _ in shapes)
    # channel counts that are no multiple of 4: kp > cin, pad columns in wt and dwt
    assert any(cin % 4 for cin, _ in shapes)


def test_integer_cases_are_exact_in_float32():
    assert 4 * 4 * ref.MAX_C == 16384 < 2 ** 24      # the products: max |x| * max |w| * cin at cin = 1024
    worst = max(max(ref.wgrad_pixels(cin, cout)) for cin, cout in ref.EXACT_SHAPES)
    assert worst == 2 * 512 + 5 and 16 * worst < 2 ** 24 and 16 * ref.FIRST_GROWN_PIXELS < 2 ** 24      # the gradient: 16 * pixels
    for cin, cout in ref.EXACT_SHAPES:
        c = ref.min_chunk(cin, cout)
        assert ref.wgrad_pixels(cin, cout) == [1, 5, 63, 64, 65, c + 1, 2 * c + 5]
        assert ref.chunk(c + 1, cin, cout) == c == ref.chunk(2 * c + 5, cin, cout)      # two and three chunks, the last one short
    cin, cout = ref.NARROWEST_WIDE
    assert (cin, cout) == (257, 3) and ref.min_chunk(cin, cout) == ref.MIN_CHUNK
    assert ref.FIRST_GROWN_PIXELS == 65537 and ref.chunk(65536, cin, cout) == 64 and ref.chunk(65537, cin, cout) == 80
    # the rounding cases: several workgroups of the products with a ragged last one, and more than one chunk where the shape allows
    assert ref.ROUNDING_PIXELS % 64 and ref.ROUNDING_PIXELS > 4 * 64
    assert -(-ref.ROUNDING_PIXELS // ref.chunk(ref.ROUNDING_PIXELS, 424, 256)) == 3
