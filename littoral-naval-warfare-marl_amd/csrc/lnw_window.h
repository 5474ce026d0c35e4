// lnw_window.h — the observation window table's record format, its packer and
// the byte -> float conversion, in plain C so that the device code, the host
// code and a stand-alone host program (tools/window_bytes_check.c) compile the
// same text.
//
// One 64-byte, 64-byte-aligned record per cell and window class holds the raw
// grid bytes of the ship's terrain window, zero padded:
//   class 0  Combatant        7x7 around the ship, rows/cols pos-3..pos+3 (49 bytes)
//   class 1  LandingShip      5x5, rows/cols pos-1..pos+3               (25 bytes)
//   class 2  medium Combatant 5x5 around the ship, pos-2..pos+2        (25 bytes)
// (combatant.py:165-181, landingship.py:178-188). A cell outside the
// hard-coded 0..99, or outside the grid, holds 0 (combatant.py:176,
// landingship.py:183). Table: [3][G*G] records, cell x*G + y.
#ifndef LNW_WINDOW_H
#define LNW_WINDOW_H
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LNW_WIN_FN __host__ __device__ static inline
#else
#define LNW_WIN_FN static inline
#endif

#define LNW_WIN_REC 64       /* bytes per record */
#define LNW_WIN_CLASSES 3

// float32(float64(b) / 255.0) for a byte b (the observation's grid/255,
// combatant.py:177), bit for bit, without a division: the product with the
// rounded reciprocal is off by one ulp for 126 of the 256 bytes, and one
// Newton step on the exact remainder (r = b - q*255 is exact in an fma)
// corrects every one of them. The fmas are explicit: the library is built with
// -ffp-contract=off.
LNW_WIN_FN float win_byte_f32(uint32_t b) {
  const float f = (float)b;
  const float q = f * (1.0f / 255.0f);
  const float r = __builtin_fmaf(-q, 255.0f, f);
  return __builtin_fmaf(r, 1.0f / 255.0f, q);
}

LNW_WIN_FN uint8_t win_cell(const uint8_t *grid, int G, int x, int y) {
  return (0 <= x && x < 100 && 0 <= y && y < 100 && x < G && y < G) ? grid[(size_t)x * G + y] : 0;
}

// The whole table from the byte grid [G][G]: out holds 3*G*G*64 bytes.
LNW_WIN_FN void win_pack_records(const uint8_t *grid, int G, uint8_t *out) {
  const size_t GG = (size_t)G * G;
  for (size_t i = 0; i < (size_t)LNW_WIN_CLASSES * GG * LNW_WIN_REC; i++) out[i] = 0;
  for (int x = 0; x < G; x++)
    for (int y = 0; y < G; y++) {
      const size_t cell = (size_t)x * G + y;
      uint8_t *w7 = out + cell * LNW_WIN_REC;
      for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) w7[i * 7 + j] = win_cell(grid, G, x - 3 + i, y - 3 + j);
      uint8_t *w5 = out + (GG + cell) * LNW_WIN_REC;
      for (int i = 0; i < 5; i++)
        for (int j = 0; j < 5; j++) w5[i * 5 + j] = win_cell(grid, G, x - 1 + i, y - 1 + j);
      uint8_t *wm = out + (2 * GG + cell) * LNW_WIN_REC;
      for (int i = 0; i < 5; i++)
        for (int j = 0; j < 5; j++) wm[i * 5 + j] = win_cell(grid, G, x - 2 + i, y - 2 + j);
    }
}

#endif
