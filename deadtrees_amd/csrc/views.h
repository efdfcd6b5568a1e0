// Dihedral views of a tile, shared by the training augmentation (elementwise.hip) and test-time augmentation (stitch.hip).
// A view is (flip: 0 none, 1 horizontal, 2 vertical; rot: k of np.rot90, counter-clockwise): view = rot90^k(flip(tile)).
#pragma once
#include "common.h"

// view[y][x] = tile[sy][sx]
__device__ __forceinline__ void aug_source_pixel(int flip, int rot, int y, int x, int H, int W, int* sy, int* sx) {
  // out = rot90^k(flip(in)):  rot90(m,1)[i][j] = m[j][N-1-i]
  int ry = y, rx = x;
  if (rot == 1) { ry = x; rx = W - 1 - y; }
  else if (rot == 2) { ry = H - 1 - y; rx = W - 1 - x; }
  else if (rot == 3) { ry = H - 1 - x; rx = y; }
  if (flip == 1) rx = W - 1 - rx;
  else if (flip == 2) ry = H - 1 - ry;
  *sy = ry;
  *sx = rx;
}
