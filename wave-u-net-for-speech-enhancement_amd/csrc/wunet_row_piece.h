// The (row, piece) walk of the row losses (wunet_loss_rows.h) and the mixer (wunet_mix.h): one block per piece of a row.
#pragma once
#include "wunet_dev.h"

// Piece `piece` of row `row`, a row being `len` samples cut into pieces of `plen` (row_pieces in wunet_ops.cpp): samples [beg, end) of
// the row, never empty.
struct RowPiece { size_t row, piece, beg, end; };
__device__ __forceinline__ RowPiece row_piece(size_t row, size_t piece, size_t plen, size_t len)
{
    const size_t beg = piece * plen;
    return RowPiece{row, piece, beg, beg + plen < len ? beg + plen : len};
}
