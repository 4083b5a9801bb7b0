"""Host-only: the room of the forward's band masks inside the binning blob (include/gsr.h gsr_binning_layout.band_masks) and the
debug bit that makes the backward blend ignore them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_band_masks_lie_inside_tile_keys_alt_behind_the_validity_bytes():
    from diff_gaussian_rasterization import _C
    for W, H in ((16, 16), (1980, 1080), (4097, 16)):   # column pairs, column pairs, tile sort
        for R in (0, 1, 2, 3, 4, 5, 63, 64, 65, 1000, 5_287_940, 9_161_997):
            bl = _C.binning_layout(1000, R, W, H)
            # the validity bytes are cleared in whole words: the masks start behind the last of those words ...
            assert bl.band_masks == bl.tile_keys_alt + 4 * ((R + 3) // 4), (W, H, R)
            # ... and end inside the array, in front of the table area
            assert bl.band_masks + R <= bl.sort_table, (W, H, R)
            # the arrays in front keep their places: four bytes per instance each, 256-byte aligned
            step = (4 * R + 255) // 256 * 256
            assert (bl.point_list, bl.point_list_alt, bl.tile_keys, bl.tile_keys_alt, bl.sort_table) == (0, step, 2 * step, 3 * step, 4 * step), (W, H, R)
            assert bl.total > bl.checkpoints >= bl.sort_table


def test_the_recompute_switch_is_a_free_bit_of_the_debug_mask():
    from diff_gaussian_rasterization import _C
    bits = {}
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        for name, v in re.findall(r"#define\s+(GSR_DEBUG_[A-Z_]+)\s+(\d+)", open(os.path.join(ROOT, "include", h)).read()):
            bits[name] = int(v)
    bit = bits["GSR_DEBUG_RECOMPUTE_BANDS"]
    assert bit == _C.DEBUG_RECOMPUTE_BANDS == 256 and bit & (bit - 1) == 0
    assert [n for n, v in bits.items() if v == bit] == ["GSR_DEBUG_RECOMPUTE_BANDS"], bits
