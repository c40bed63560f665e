// srd_rows.hip -- keyed reads into fixed-size rows with no host wait
// (srd_read_rows_device; host glue in srd_ops.hip).
//
// Reference being replaced (jzombie/rust-simd-r-drive v0.16.3-alpha): a batch
// read whose handles are copied out and checked --
//   batch_read_hashed_keys                   src/storage_engine/data_store.rs:1111-1158
//   read_entry_with_context                  src/storage_engine/data_store.rs:502-565
//   EntryHandle::as_slice / is_valid_checksum
//                       simd-r-drive-entry-handle/src/entry_handle.rs:260-275
//
// The gather (srd_gather.hip) with the look-up in front and a destination
// known by arithmetic: query i goes to row i of the caller's [n, row_stride]
// buffer, so nothing of the layout has to reach the host.  The unit counts'
// exclusive sum stays on the device; the unit kernels and the streaming kernel
// run in their device-count forms (srd_units.hip, srd_stream.hip) on grids
// sized from the bound rows_units_bound (srd_rows.h).  Steps, all on the
// caller's stream:
//   rows_begin_kernel    the counters at 0
//   rows_layout_kernel   per query: probe, tag check, entry_range, rows_judge;
//                        the range view of the batch (then one hipCUB
//                        exclusive sum over n + 1 unit counts: upre[n] is the
//                        unit total)
//   units_kernel .. unit_combine_kernel   as the gather's, the count from upre[n]
//   rows_finish_kernel   per query: stored checksum, status, length, CRC, counts

namespace srd {

// (the rows as UnitArgs' ranges: eun = the unit counts, eun[n] = 0; off[i] =
// i * row_stride; upre = the exclusive sum of eun[0 .. n], upre[n] the total)
struct RowsArgs : UnitArgs {
  Table t;
  uint64_t flen;
  const uint64_t* q;       // [n] key hashes
  const uint64_t* verify;  // [n] nullable: the hashes whose tags the entries must carry
  uint64_t row_stride, row_cap;
  uint64_t *o_start, *o_end;  // [n] the workspace behind UnitArgs::start / end
  uint8_t* st;                // [n] rows_judge's status
  unsigned long long* cnt;    // [0] the rows of more than one unit
  // the caller's arrays (rows_finish_kernel)
  uint64_t* o_len;
  uint8_t* o_status;
  uint32_t* o_crc;
  unsigned long long* o_counts;  // [ROWS_STATUSES] nullable, zeroed by rows_begin_kernel
};

// The call's two counters at their start values, by a kernel of the chain
// itself: the multi-unit count of the workspace and the caller's status counts.
__global__ void rows_begin_kernel(unsigned long long* cnt, unsigned long long* o_counts) {
  if (threadIdx.x == 0) cnt[0] = 0;
  if (o_counts && threadIdx.x < ROWS_STATUSES) o_counts[threadIdx.x] = 0;
}

// One lane per query: batch_read_kernel's decision (srd_index.hip) and
// payload_layout_kernel's in one pass, with nothing between them in memory.  A
// row that is not delivered has no units; a TOO_LONG row keeps its range (its
// length is end - start), a NONE row gets (0, 0).
__global__ __launch_bounds__(256) void rows_layout_kernel(RowsArgs a) {
  unsigned long long multi = 0;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i <= a.n; i += gridDim.x * 256ull) {
    if (i == a.n) {  // the addend behind the last row: its prefix is the unit total
      a.eun[i] = 0;
      continue;
    }
    uint64_t start = 0, end = 0;
    const uint64_t p = table_get(a.t, a.q[i]);
    bool have = p != TBL_EMPTY;
    if (have && a.verify) have = (p >> 48) == (a.verify[i] >> 48);  // tag_from_key(non_hashed_key), :513-521
    if (have) have = entry_range(a.file, a.flen, p & 0xFFFFFFFFFFFFull, &start, &end);
    const RowVerdict v = rows_judge(start, end, have, a.row_cap);
    a.o_start[i] = v.status == SRD_GATHER_NONE ? 0 : start;
    a.o_end[i] = v.status == SRD_GATHER_NONE ? 0 : end;
    a.eun[i] = v.units;
    a.off[i] = i * a.row_stride;
    a.st[i] = (uint8_t)v.status;
    multi += v.units > 1;
  }
  // a wave reduction, the block's four waves through LDS, one atomic per block
  // (iter_flag_kernel's shape)
  __shared__ unsigned long long part[4];
  for (int o = 32; o > 0; o >>= 1) multi += __shfl_xor(multi, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = multi;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long sum = part[0] + part[1] + part[2] + part[3];
    if (sum) atomicAdd(a.cnt, sum);
  }
}

// Per query: the stored checksum -- the little-endian u32 at end + 16, inside
// the file by entry_range -- against the computed one; status, length and CRC
// into the caller's arrays, and the statuses counted (here, where OK and
// BAD_CRC are told apart): one atomic per block and status that occurred.
__global__ __launch_bounds__(256) void rows_finish_kernel(RowsArgs a) {
  unsigned long long c[ROWS_STATUSES] = {};
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < a.n; i += gridDim.x * 256ull) {
    uint32_t st = a.st[i], crc = 0;
    if (st == SRD_GATHER_OK) {
      crc = a.crc[i];
      if (crc != ld_u32_unaligned(a.file, a.end[i] + 16)) st = SRD_GATHER_BAD_CRC;
    }
    a.o_status[i] = (uint8_t)st;
    a.o_len[i] = a.end[i] - a.start[i];
    if (a.o_crc) a.o_crc[i] = crc;
#pragma unroll
    for (uint32_t s = 0; s < ROWS_STATUSES; s++) c[s] += st == s;
  }
  if (!a.o_counts) return;
  __shared__ unsigned long long part[4][ROWS_STATUSES];
#pragma unroll
  for (uint32_t s = 0; s < ROWS_STATUSES; s++) {
    for (int o = 32; o > 0; o >>= 1) c[s] += __shfl_xor(c[s], o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][s] = c[s];
  }
  __syncthreads();
  if (threadIdx.x < ROWS_STATUSES) {
    const unsigned long long sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (sum) atomicAdd(a.o_counts + threadIdx.x, sum);
  }
}

}  // namespace srd
