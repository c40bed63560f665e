// srd_rows.h -- the arithmetic of srd_read_rows_device:
// how a looked-up entry becomes a row's status, length and unit count
// (rows_judge), the bound on a batch's work units that sizes grids and
// workspace without a read-back (rows_units_bound), the refusals the host
// decides by arithmetic before anything is enqueued (rows_refusal), and the
// workspace sizes.  Plain integer code shared by the kernels (srd_rows.hip),
// the host glue (srd_ops.hip) and a CPU check
// (tests/sanitize_rows/rows_check.cpp): outside HIP the qualifiers are empty.
//
// Row i of the output is the bytes [i * row_stride, i * row_stride + row_cap)
// from d_out.  d_out is 16-byte aligned and row_stride a multiple of 16, so a
// row starts at a 16-byte boundary and a delivered entry is cut exactly like a
// hit of the gather (the range view of srd_segments.h with off[i] = i *
// row_stride, pad = false): chunk j of it is the unit upre[i] + j.
#pragma once
#include <stdint.h>

#include "srd_gather.h"
#include "srd_segments.h"

namespace srd {

constexpr uint32_t ROWS_TOO_LONG = SRD_ROWS_TOO_LONG;
static_assert(ROWS_TOO_LONG == 5 && SRD_GATHER_NONE == 0 && SRD_GATHER_OK == 1 && SRD_GATHER_BAD_CRC == 2,
              "the row statuses keep the gather's values; 3 cannot arise, 4 is the scatter's");
constexpr uint64_t ROWS_STATUSES = 6;  // d_counts: one word per status value 0 .. 5

// One query: `have` = the key is indexed, its tag agrees and entry_range gave
// [start, end).  NONE: no entry (length 0).  TOO_LONG: the entry does not fit a
// row -- its true length is reported, nothing of it is read or written.
// Otherwise it is delivered (reported as OK here; the checksum turns it into
// OK or BAD_CRC) in gather_chunks(len) units.
struct RowVerdict {
  uint32_t status;
  uint64_t len, units;
};
SRD_GA_HD RowVerdict rows_judge(uint64_t start, uint64_t end, bool have, uint64_t row_cap) {
  if (!have || start >= end) return RowVerdict{SRD_GATHER_NONE, 0, 0};
  const uint64_t len = end - start;
  if (len > row_cap) return RowVerdict{ROWS_TOO_LONG, len, 0};
  return RowVerdict{SRD_GATHER_OK, len, gather_chunks(len)};
}

// ceil(row_cap / C) without an addition that could wrap: the most units a row can have
SRD_GA_HD uint64_t rows_units_per_row(uint64_t row_cap) { return row_cap / GATHER_CHUNK + (row_cap % GATHER_CHUNK != 0); }
// n * ceil(row_cap / C): false when the product does not fit 64 bits
SRD_GA_HD bool rows_units_bound(uint64_t n, uint64_t row_cap, uint64_t* bound) {
  const uint64_t per = rows_units_per_row(row_cap);
  if (n && per > ~0ull / n) return false;
  *bound = n * per;
  return true;
}

// What the host refuses before anything is enqueued: nullptr, or the message.
struct RowsCall {
  uint64_t file, file_padded;  // d_file and srd_padded_size(file_len)
  uint64_t out, n, row_stride, row_cap;
  uint32_t flags;
  bool ptrs;  // every required pointer is there
};
SRD_GA_HD const char* rows_refusal(const RowsCall& r) {
  if (r.flags) return "bad argument: flags must be 0";
  if (r.n >= (1ull << 31)) return "too many queries in one batch";
  if (!r.n) return nullptr;  // (runs nothing)
  if (!r.ptrs) return "bad argument: a required pointer is NULL";
  if (r.out & 15) return "bad argument: d_out must be 16-byte aligned";
  if (!r.row_cap) return "bad argument: row_cap must be at least 1";
  if (r.row_stride & 15) return "bad argument: row_stride must be a multiple of 16";
  if (r.row_stride < r.row_cap) return "bad argument: row_stride is below row_cap";
  uint64_t bound = 0;
  if (!rows_units_bound(r.n, r.row_cap, &bound) || bound >= (1ull << 32)) return "too many work units in one batch";
  if (r.row_stride > ~0ull / r.n) return "bad argument: n * row_stride does not fit 64 bits";
  const uint64_t bytes = r.n * r.row_stride;
  if (bytes > ~0ull - r.out) return "bad argument: the rows do not fit the address space";
  // [out, out + bytes) against [file, file + file_padded): no sum that could wrap
  if (r.file_padded && r.out < r.file + r.file_padded && (r.file <= r.out || r.file - r.out < bytes))
    return "d_out overlaps the store";
  return nullptr;
}

// The workspace of a call of (n, row_cap), in bytes: the per-query arrays of 8,
// 4 and 1 bytes (the 8-byte ones one element longer: the unit counts end in a
// 0 whose prefix is the batch's unit total), the unit table and the units' raw
// CRCs for the bound.  Monotone in n and in row_cap.  (n < 2^31 and a bound
// below 2^32: nothing wraps.)
SRD_GA_HD uint64_t rows_ws_u64(uint64_t n) { return (n + 1) * 8; }
SRD_GA_HD uint64_t rows_ws_u32(uint64_t n) { return n * 4; }
SRD_GA_HD uint64_t rows_ws_u8(uint64_t n) { return n; }
SRD_GA_HD uint64_t rows_ws_units(uint64_t bound) { return bound * sizeof(SegUnit); }
SRD_GA_HD uint64_t rows_ws_raw(uint64_t bound) { return bound * 4; }

}  // namespace srd
