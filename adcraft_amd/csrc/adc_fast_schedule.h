// adc_fast_schedule.h - how k_step_implicit_fast (parts/kernel_fast.inc) deals a tile's auctions to its lanes: the arithmetic
// of phase 2's schedule, shared with its host twin adc_fast_schedule_host (adc_shims.cpp).  Nothing here touches the stream:
// every draw is addressed by (auction, keyword, tick), so the mapping of auctions to lanes is free, and this file only decides
// how many issue slots the mapping costs.
//
// A tile is resolved in three passes of one Philox call = four auctions per lane and slot:
//   pass 0  FULL ITEMS      `chunk` = 1 << chunk_shift consecutive auctions of one keyword (chunk / 4 calls), V >> chunk_shift per keyword
//   pass 1  TAIL CALLS      the whole calls among a keyword's last V mod chunk auctions: ((V mod chunk) >> 2) items of one call
//   pass 2  PARTIAL CALLS   the keyword's last V mod 4 auctions, one keyword per lane, one call
// Passes 0 and 1 deal their items (numbered by an exclusive prefix over the keywords) lane-major and PER WAVE: the tile's
// ceil(total / 64) wave-rounds are split over the four waves as evenly as whole rounds allow (R_w, differing by at most one),
// part w owns the items from 64 * (rounds of the parts before it), lane l of it the R_w consecutive items from base_w + l R_w;
// which wave takes which part rotates with the tile's index.
// A workgroup-wide round count would make all four waves run ceil(total / 256) rounds - up to three wave-rounds of empty slots.
#pragma once
#include "adc_law.h"

namespace adc {

constexpr int kFastTileLanes = 256;             // lanes of a workgroup = keywords of a full tile
constexpr int kFastWaveLanes = 64;
constexpr int kFastTileWaves = kFastTileLanes / kFastWaveLanes;
static_assert((kFastTileWaves & (kFastTileWaves - 1)) == 0, "fast_wave_part masks with kFastTileWaves - 1");
constexpr int kFastCallShift = 2;               // one Philox call serves four auctions
constexpr int kDenseVolumePerKeyword = 24;      // tiles averaging at least this many auctions per non-empty keyword use intervals

// the form a tile is resolved in (tile_live = keywords with auctions): word intervals, or auction by auction (DIRECT)
ADC_HD bool fast_tile_dense(int tile_volume, int tile_live) { return tile_volume >= kDenseVolumePerKeyword * tile_live; }

// work-item size of pass 0: 16 auctions when the tile has plenty of them; 8 or 4 on sparse tiles, so that the items still
// number about two per lane
ADC_HD int fast_chunk_shift(int tile_volume)
{
    return tile_volume >= 32 * kFastTileLanes ? 4 : tile_volume >= 16 * kFastTileLanes ? 3 : 2;
}

// per keyword: items of pass 0 and pass 1, and where each pass starts in the keyword's auctions
ADC_HD int fast_full_items(int V, int chunk_shift) { return V >> chunk_shift; }
ADC_HD int fast_tail_calls(int V, int chunk_shift) { return (V & ((1 << chunk_shift) - 1)) >> kFastCallShift; }
ADC_HD int fast_tail_first(int V, int chunk_shift) { return (V >> chunk_shift) << chunk_shift; }
ADC_HD int fast_partial_first(int V) { return (V >> kFastCallShift) << kFastCallShift; }
ADC_HD int fast_partial_count(int V) { return V & ((1 << kFastCallShift) - 1); }
constexpr int kFastTailCallsMax = 3;            // (chunk <= 16: a tail of at most 15 auctions)
// full items and tail calls of a keyword in one word, so that one prefix scan over a wave's 64 keywords serves both: the wave's
// full items stay below 2^23 (items of 16: 64 keywords x 2^20 / 16 = 2^22; smaller items only in tiles of fewer than 8192
// auctions), its tail calls below 2^8
constexpr int kFastPackShift = 23;
ADC_HD int fast_pack_counts(int full_items, int tail_calls) { return full_items | (tail_calls << kFastPackShift); }
ADC_HD int fast_packed_items(int packed) { return packed & ((1 << kFastPackShift) - 1); }
ADC_HD int fast_packed_calls(int packed) { return packed >> kFastPackShift; }
ADC_HD int fast_calls_needed(int V) { return (V + (1 << kFastCallShift) - 1) >> kFastCallShift; }       // calls that hold an auction

// passes 0 and 1, `total` items: the range is cut in four contiguous parts; part p runs fast_wave_rounds(total, p) rounds from
// item fast_wave_base(total, p) (the first total % 4 parts one round more than the others).  Wave w of the workgroup takes part
// (w + tile index) mod 4: with the parts fixed to the waves, the short parts would fall to the same wave of every workgroup, and
// the hardware places a workgroup's four waves on the CU's four SIMDs in order - one SIMD would get all the relief.
ADC_HD int fast_wave_part(int w, int tile_index) { return (w + tile_index) & (kFastTileWaves - 1); }
ADC_HD int fast_wave_rounds(int total, int w)
{
    const int wave_rounds = (total + kFastWaveLanes - 1) / kFastWaveLanes;
    return wave_rounds / kFastTileWaves + (w < wave_rounds % kFastTileWaves ? 1 : 0);
}
ADC_HD int fast_wave_base(int total, int w)
{
    const int wave_rounds = (total + kFastWaveLanes - 1) / kFastWaveLanes;
    const int q = wave_rounds / kFastTileWaves, r = wave_rounds % kFastTileWaves;
    return kFastWaveLanes * (w * q + (w < r ? w : r));
}
// a lane whose wave starts at `base` and runs `rounds` rounds owns the items [first, first + rounds) clipped to `total`: round r
// of it has the item first + r if that exists
ADC_HD int fast_lane_first(int base, int rounds, int lane, int total)
{
    const int first = base + lane * rounds;
    return first < total ? first : total;
}
ADC_HD bool fast_item_exists(int item, int total) { return item < total; }

}  // namespace adc
