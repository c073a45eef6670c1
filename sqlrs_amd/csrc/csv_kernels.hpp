// csv_kernels.hpp — the device form of the CSV reader (csv_device.hip): bytes of one piece of the file -> columns.  The piece is
// quote-free, or (sqlrs_csv_set_device_quotes) its quotes are all regular: "quoted fields" below.
//
//   classify   16 bytes per lane, 4096 per workgroup: which bytes are separators (a delimiter, or a '\n' that ends a
//              record — a '\n' that ends a blank line is none), their count per tile, "a '"' was seen"
//   index      tile counts scanned (scan.hip) -> every separator's rank f and byte position; separator f ends field f,
//              row f / C, column f % C — valid while every '\n' has f % C = C - 1 and no delimiter has: the first
//              violation's row (atomicMin) is the ragged record, every row before it is good
//   parse      one lane per (row, projected column): Int64 / Float64 / Boolean -> 8 value bytes + a validity byte;
//              Utf8 -> start and length in the piece.  A Float64 field outside the exactly rounded rule goes on the patch
//              list (the host writes it with std::from_chars), an unparsable field lowers the piece's error row
//   cut / pack rows [a, b) of the piece appended to the batch under construction (values, Utf8 offsets and bytes, one flag
//              byte per row), the flag bytes of a finished batch -> validity / Boolean bitmaps, one ballot word per wave
#pragma once

#include "common.hpp"
#include "device_utils.hpp"

namespace sq {

constexpr int CSV_WG = 256;
constexpr int CSV_LANE_BYTES = 16;
constexpr int CSV_TILE = CSV_WG * CSV_LANE_BYTES;
constexpr int CSV_MAX_SLOTS = 32; // projected columns per launch (the parameter block holds their descriptors)
constexpr uint32_t CSV_NO_ROW = 0xffffffffu;
constexpr uint32_t CSV_ESCAPES = 0x80000000u; // (a piece is shorter than 2^31 - 64 bytes)
constexpr int CSV_NULL_BANKS = 8; // counters per (output batch, column) that the NULL counts are spread over

// control words of one piece (device, zeroed / preset before the kernels)
struct CsvCtl {
  uint32_t quote;       // a '"' byte anywhere in the piece
  uint32_t first_bad;   // row of the first separator that breaks the f % C rule (CSV_NO_ROW: none)
  uint32_t err_row;     // first row with an unparsable typed field (CSV_NO_ROW: none)
  uint32_t num_patches; // entries on the patch list
  // ---- sqlrs_csv_set_device_quotes (csv_index_q_kernel)
  uint32_t bad_quote;     // position of the first irregular quote (CSV_NO_ROW: none)
  uint32_t last_end_pos;  // position of the last '\n' that ends a record outside quotes (0: none — a '\n' at 0 ends a blank line)
  uint32_t last_end_rank; // ... and its rank among the separators
  uint32_t pad_;
};
struct CsvPatch {
  uint32_t row, slot, start, len;
};
struct CsvSlot {
  int32_t src;     // the file's column
  int32_t dtype;
  uint64_t *val;   // typed: 8 value bytes per row of the piece (Boolean: 0 / 1)
  uint8_t *flag;   // typed: 1 = valid
  uint32_t *ustart; // Utf8: first byte of the field in the piece (CSV_ESCAPES set: a quoted field with "" pairs inside)
  uint32_t *ulen;   // Utf8: its length, a "" pair counted once; [rows] = 0 (scanned into uoff[rows + 1])
  const uint32_t *uoff;
};
struct CsvParams {
  int nslots, C;
  int64_t rows;         // rows of the piece that are parsed
  int64_t seg_first, B; // rows [0, seg_first) finish the batch under construction, then batches of B rows
  CsvSlot slot[CSV_MAX_SLOTS];
};
// a batch under construction, one per projected column
struct CsvOut {
  uint64_t *values;  // Int64 / Float64: 8 bytes per row; Boolean: the bitmap (written by pack)
  uint64_t *validity;
  int32_t *offsets;  // Utf8
  uint8_t *bytes;
  uint8_t *vb;       // staging: bit 0 valid, bit 1 Boolean value, one byte per row
  uint32_t ubase;    // Utf8 bytes already in the batch
};
struct CsvOutParams {
  CsvOut out[CSV_MAX_SLOTS];
};

// The lane's 16 bytes at i0: bit k of `delims` = byte i0 + k is the delimiter, of `ends` = it is a '\n' that ends a record.
// A '\n' ends a blank line, and is no separator, when the byte before it — one '\r' skipped — is a '\n' or the start of the data.
__device__ __forceinline__ void csv_masks16(const uint8_t *__restrict__ b, int64_t n, int64_t i0, uint8_t delim, uint32_t &delims,
                                            uint32_t &ends, bool &quote) {
  delims = ends = 0;
  quote = false;
  if (i0 >= n) return;
  const uint4 q = *(const uint4 *)(b + i0); // (the buffer is padded to whole 16 bytes)
  uint8_t w[CSV_LANE_BYTES + 2];
  w[0] = i0 >= 2 ? b[i0 - 2] : (uint8_t)'\n';
  w[1] = i0 >= 1 ? b[i0 - 1] : (uint8_t)'\n';
  const uint32_t qs[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int k = 0; k < CSV_LANE_BYTES; k++) w[k + 2] = (uint8_t)(qs[k >> 2] >> (8 * (k & 3)));
  uint32_t quotes = 0;
#pragma unroll
  for (int k = 0; k < CSV_LANE_BYTES; k++) {
    const uint8_t c = w[k + 2];
    const bool blank = w[k + 1] == '\n' || (w[k + 1] == '\r' && w[k] == '\n');
    delims |= (uint32_t)(c == delim) << k;
    ends |= (uint32_t)(c == '\n' && c != delim && !blank) << k;
    quotes |= (uint32_t)(c == '"') << k;
  }
  const uint32_t live = n - i0 >= CSV_LANE_BYTES ? 0xffffu : (1u << (int)(n - i0)) - 1; // bytes behind the piece's end are not its
  delims &= live;
  ends &= live;
  quote = (quotes & live) != 0;
}

__global__ __launch_bounds__(CSV_WG) void csv_classify_kernel(const uint8_t *__restrict__ b, int64_t n, uint8_t delim,
                                                              uint32_t *__restrict__ tile_cnt, CsvCtl *__restrict__ ctl) {
  __shared__ uint32_t s_wave[CSV_WG / 64];
  const int64_t i0 = ((int64_t)blockIdx.x * CSV_WG + threadIdx.x) * CSV_LANE_BYTES;
  uint32_t delims, ends;
  bool quote;
  csv_masks16(b, n, i0, delim, delims, ends, quote);
  const uint32_t cnt = wave_sum_u32((uint32_t)__popc(delims | ends));
  const bool any_quote = __ballot(quote) != 0;
  if (lane_id() == 0) {
    s_wave[threadIdx.x >> 6] = cnt;
    if (any_quote) atomicOr(&ctl->quote, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

__global__ __launch_bounds__(CSV_WG) void csv_index_kernel(const uint8_t *__restrict__ b, int64_t n, uint8_t delim, uint32_t C,
                                                           const uint32_t *__restrict__ tile_off, uint32_t *__restrict__ sep_pos,
                                                           CsvCtl *__restrict__ ctl) {
  __shared__ uint32_t s_wave[CSV_WG / 64];
  const int64_t i0 = ((int64_t)blockIdx.x * CSV_WG + threadIdx.x) * CSV_LANE_BYTES;
  uint32_t delims, ends;
  bool quote;
  csv_masks16(b, n, i0, delim, delims, ends, quote);
  const uint32_t cnt = (uint32_t)__popc(delims | ends);
  const uint32_t incl = wave_iscan_u32(cnt);
  const int w = threadIdx.x >> 6;
  if (lane_id() == 63) s_wave[w] = incl;
  __syncthreads();
  uint32_t rank = tile_off[blockIdx.x] + incl - cnt;
  for (int k = 0; k < w; k++) rank += s_wave[k];
  uint32_t seps = delims | ends, bad_row = CSV_NO_ROW;
  while (seps) {
    const int k = __ffs(seps) - 1;
    seps &= seps - 1;
    sep_pos[rank] = (uint32_t)(i0 + k);
    const bool last_col = rank % C == C - 1, is_end = (ends >> k) & 1;
    if (last_col != is_end) bad_row = min(bad_row, rank / C);
    rank++;
  }
  if (bad_row != CSV_NO_ROW) atomicMin(&ctl->first_bad, bad_row);
}

// ---- quoted fields (sqlrs_csv_set_device_quotes) ---------------------------------------------------------------------------------
// Every '"' toggles "inside quotes"; par(i) = number of quotes in [0, i) mod 2, and a piece starts outside.  That is what the
// host parser reads exactly when every quote is REGULAR: one with par = 0 (it opens) is the piece's first byte or follows the
// delimiter, a '\n' or a quote (which closed: an escaped pair); one with par = 1 (it closes) is followed by the delimiter,
// '\n', "\r\n" or a quote.  The kernels find the separators outside quotes and the first irregular quote; a piece with one in
// front of its last record end is the host parser's.
//
//   quotes     '"' bytes per tile; scanned, the low bit is the tile's starting parity
//   classify_q / index_q   csv_classify / csv_index with delimiters and record ends inside quotes masked out; index_q also
//              checks the two regularity rules and keeps the last record end outside quotes: the piece is cut there

// the lane's 16 bytes: bit k = byte i0 + k is a '"'
__device__ __forceinline__ uint32_t csv_quotes16(const uint8_t *__restrict__ b, int64_t n, int64_t i0) {
  if (i0 >= n) return 0;
  const uint4 q = *(const uint4 *)(b + i0);
  const uint32_t qs[4] = {q.x, q.y, q.z, q.w};
  uint32_t quotes = 0;
#pragma unroll
  for (int k = 0; k < CSV_LANE_BYTES; k++) quotes |= (uint32_t)((uint8_t)(qs[k >> 2] >> (8 * (k & 3))) == '"') << k;
  return quotes & (n - i0 >= CSV_LANE_BYTES ? 0xffffu : (1u << (int)(n - i0)) - 1);
}

__global__ __launch_bounds__(CSV_WG) void csv_quotes_kernel(const uint8_t *__restrict__ b, int64_t n, uint32_t *__restrict__ tile_quotes) {
  __shared__ uint32_t s_wave[CSV_WG / 64];
  const int64_t i0 = ((int64_t)blockIdx.x * CSV_WG + threadIdx.x) * CSV_LANE_BYTES;
  const uint32_t cnt = wave_sum_u32((uint32_t)__popc(csv_quotes16(b, n, i0)));
  if (lane_id() == 0) s_wave[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) tile_quotes[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// csv_masks16 outside quotes.  `delims` / `ends` are the separators with par = 0; `bad` the irregular quotes of the lane.
// Every lane of the workgroup calls it (a barrier inside); s_par holds one word per wave.
__device__ __forceinline__ void csv_masks16_q(const uint8_t *__restrict__ b, int64_t n, int64_t i0, uint8_t delim, uint32_t tile_par,
                                              uint32_t *s_par, uint32_t &delims, uint32_t &ends, uint32_t &bad) {
  uint32_t quotes = 0, open_ok = 0, close_ok = 0;
  delims = ends = 0;
  if (i0 < n) {
    const uint4 q = *(const uint4 *)(b + i0); // (the buffer is padded to whole 16 bytes, and 16 more)
    uint8_t w[CSV_LANE_BYTES + 4];
    w[0] = i0 >= 2 ? b[i0 - 2] : (uint8_t)'\n';
    w[1] = i0 >= 1 ? b[i0 - 1] : (uint8_t)'\n';
    w[CSV_LANE_BYTES + 2] = i0 + CSV_LANE_BYTES < n ? b[i0 + CSV_LANE_BYTES] : (uint8_t)0; // (a piece ends in '\n': no quote of it looks further)
    w[CSV_LANE_BYTES + 3] = i0 + CSV_LANE_BYTES + 1 < n ? b[i0 + CSV_LANE_BYTES + 1] : (uint8_t)0;
    const uint32_t qs[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < CSV_LANE_BYTES; k++) w[k + 2] = (uint8_t)(qs[k >> 2] >> (8 * (k & 3)));
#pragma unroll
    for (int k = 0; k < CSV_LANE_BYTES; k++) {
      const uint8_t c = w[k + 2], p = w[k + 1], x = w[k + 3];
      const bool blank = p == '\n' || (p == '\r' && w[k] == '\n');
      delims |= (uint32_t)(c == delim) << k;
      ends |= (uint32_t)(c == '\n' && c != delim && !blank) << k;
      quotes |= (uint32_t)(c == '"') << k;
      open_ok |= (uint32_t)(p == delim || p == '\n' || p == '"') << k; // (the byte in front of the piece reads as '\n')
      close_ok |= (uint32_t)(x == delim || x == '\n' || x == '"' || (x == '\r' && w[k + 4] == '\n')) << k;
    }
    const uint32_t live = n - i0 >= CSV_LANE_BYTES ? 0xffffu : (1u << (int)(n - i0)) - 1;
    delims &= live;
    ends &= live;
    quotes &= live;
  }
  // parity in front of the lane: the tile's, the earlier waves', the earlier lanes' of this wave
  const uint64_t odd = __ballot(__popc(quotes) & 1);
  const int wv = threadIdx.x >> 6;
  if (lane_id() == 0) s_par[wv] = (uint32_t)__popcll(odd);
  __syncthreads();
  uint32_t par = tile_par + (uint32_t)mbcnt(odd);
  for (int k = 0; k < wv; k++) par += s_par[k];
  // bit k of inq = par(i0 + k): the prefix XOR of the quote mask, exclusive, on top of the lane's starting parity
  uint32_t x = quotes;
  x ^= x << 1;
  x ^= x << 2;
  x ^= x << 4;
  x ^= x << 8;
  const uint32_t inq = ((x ^ quotes) ^ ((par & 1) ? 0xffffu : 0u)) & 0xffffu;
  delims &= ~inq & ~quotes; // (a '"' delimiter: the host side does not come here)
  ends &= ~inq;
  bad = quotes & ((~inq & ~open_ok) | (inq & ~close_ok));
}

__global__ __launch_bounds__(CSV_WG) void csv_classify_q_kernel(const uint8_t *__restrict__ b, int64_t n, uint8_t delim,
                                                                const uint32_t *__restrict__ tile_qoff, uint32_t *__restrict__ tile_cnt) {
  __shared__ uint32_t s_par[CSV_WG / 64], s_wave[CSV_WG / 64];
  const int64_t i0 = ((int64_t)blockIdx.x * CSV_WG + threadIdx.x) * CSV_LANE_BYTES;
  uint32_t delims, ends, bad;
  csv_masks16_q(b, n, i0, delim, tile_qoff[blockIdx.x], s_par, delims, ends, bad);
  const uint32_t cnt = wave_sum_u32((uint32_t)__popc(delims | ends));
  if (lane_id() == 0) s_wave[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m, 64));
  return v;
}

__global__ __launch_bounds__(CSV_WG) void csv_index_q_kernel(const uint8_t *__restrict__ b, int64_t n, uint8_t delim, uint32_t C,
                                                             const uint32_t *__restrict__ tile_qoff, const uint32_t *__restrict__ tile_off,
                                                             uint32_t *__restrict__ sep_pos, CsvCtl *__restrict__ ctl) {
  __shared__ uint32_t s_par[CSV_WG / 64], s_wave[CSV_WG / 64];
  const int64_t i0 = ((int64_t)blockIdx.x * CSV_WG + threadIdx.x) * CSV_LANE_BYTES;
  uint32_t delims, ends, bad;
  csv_masks16_q(b, n, i0, delim, tile_qoff[blockIdx.x], s_par, delims, ends, bad);
  const uint32_t cnt = (uint32_t)__popc(delims | ends);
  const uint32_t incl = wave_iscan_u32(cnt);
  const int w = threadIdx.x >> 6;
  if (lane_id() == 63) s_wave[w] = incl;
  __syncthreads();
  uint32_t rank = tile_off[blockIdx.x] + incl - cnt;
  for (int k = 0; k < w; k++) rank += s_wave[k];
  uint32_t seps = delims | ends, bad_row = CSV_NO_ROW, end_pos = 0, end_rank = 0;
  while (seps) {
    const int k = __ffs(seps) - 1;
    seps &= seps - 1;
    sep_pos[rank] = (uint32_t)(i0 + k);
    const bool last_col = rank % C == C - 1, is_end = (ends >> k) & 1;
    if (last_col != is_end) bad_row = min(bad_row, rank / C);
    if (is_end) {
      end_pos = (uint32_t)(i0 + k);
      end_rank = rank;
    }
    rank++;
  }
  if (bad_row != CSV_NO_ROW) atomicMin(&ctl->first_bad, bad_row);
  // one atomic per wave: positions and ranks grow together, so the two maxima belong to the same separator
  const uint32_t wave_bad = wave_min_u32(bad ? (uint32_t)(i0 + __ffs(bad) - 1) : CSV_NO_ROW);
  const uint32_t wave_end = wave_max_u32(end_pos), wave_rank = wave_max_u32(end_rank);
  if (lane_id() == 0) {
    if (wave_bad != CSV_NO_ROW) atomicMin(&ctl->bad_quote, wave_bad);
    if (wave_end) {
      atomicMax(&ctl->last_end_pos, wave_end);
      atomicMax(&ctl->last_end_rank, wave_rank);
    }
  }
}

__device__ const double csv_pow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                         1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

enum CsvFieldResult { CSV_FIELD_OK = 0, CSV_FIELD_ERROR = 1, CSV_FIELD_PATCH = 2 };

__device__ __forceinline__ bool csv_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// std::from_chars<int64_t>: optional '-', digits, nothing else; out of range is an error
__device__ inline int csv_parse_int64(const uint8_t *p, const uint8_t *e, uint64_t &out) {
  const bool neg = p < e && *p == '-';
  if (neg) p++;
  if (p == e) return CSV_FIELD_ERROR;
  uint64_t acc = 0;
  for (; p < e; p++) {
    if (!csv_digit(*p)) return CSV_FIELD_ERROR;
    const uint64_t d = (uint64_t)(*p - '0');
    if (acc > (0xffffffffffffffffull - d) / 10) return CSV_FIELD_ERROR;
    acc = acc * 10 + d;
  }
  if (acc > (neg ? 0x8000000000000000ull : 0x7fffffffffffffffull)) return CSV_FIELD_ERROR;
  out = neg ? 0ull - acc : acc;
  return CSV_FIELD_OK;
}

// -?digits[.digits][(e|E)[-]digits] with the digits an integer m < 2^53 and the decimal exponent k, the point moved behind
// the last digit, |k| <= 22: m and 10^|k| are exact doubles, ONE IEEE multiply or divide is the correctly rounded value.
// Anything else — also what is no number at all — is left to the host's std::from_chars.
__device__ inline int csv_parse_float64(const uint8_t *p, const uint8_t *e, uint64_t &out) {
  const bool neg = p < e && *p == '-';
  if (neg) p++;
  uint64_t m = 0;
  int nint = 0, nfrac = 0;
  for (; p < e && csv_digit(*p); p++, nint++) {
    m = m * 10 + (uint64_t)(*p - '0');
    if (m >= (1ull << 53)) return CSV_FIELD_PATCH;
  }
  if (nint == 0) return CSV_FIELD_PATCH;
  if (p < e && *p == '.') {
    p++;
    for (; p < e && csv_digit(*p); p++, nfrac++) {
      m = m * 10 + (uint64_t)(*p - '0');
      if (m >= (1ull << 53)) return CSV_FIELD_PATCH;
    }
    if (nfrac == 0) return CSV_FIELD_PATCH;
  }
  int ex = 0;
  if (p < e && (*p == 'e' || *p == 'E')) {
    p++;
    const bool eneg = p < e && *p == '-';
    if (eneg) p++;
    if (p == e) return CSV_FIELD_PATCH;
    for (; p < e; p++) {
      if (!csv_digit(*p)) return CSV_FIELD_PATCH;
      ex = ex * 10 + (*p - '0');
      if (ex > 9999) return CSV_FIELD_PATCH;
    }
    if (eneg) ex = -ex;
  }
  if (p != e) return CSV_FIELD_PATCH;
  const int k = ex - nfrac;
  if (k < -22 || k > 22) return CSV_FIELD_PATCH;
  double v = (double)(int64_t)m;
  v = k >= 0 ? v * csv_pow10[k] : v / csv_pow10[-k];
  out = (uint64_t)__double_as_longlong(neg ? -v : v);
  return CSV_FIELD_OK;
}

__device__ __forceinline__ uint8_t csv_lower(uint8_t c) { return c >= 'A' && c <= 'Z' ? (uint8_t)(c + 32) : c; }
__device__ inline int csv_parse_bool(const uint8_t *p, const uint8_t *e, uint64_t &out) {
  const int len = (int)(e - p);
  const char *t = len == 4 ? "true" : "false";
  if (len != 4 && len != 5) return CSV_FIELD_ERROR;
  for (int k = 0; k < len; k++)
    if (csv_lower(p[k]) != (uint8_t)t[k]) return CSV_FIELD_ERROR;
  out = len == 4;
  return CSV_FIELD_OK;
}

// segment (= output batch) of a row of the piece
__device__ __forceinline__ uint32_t csv_segment(int64_t row, int64_t seg_first, int64_t B) {
  return row < seg_first ? 0u : 1u + (uint32_t)((row - seg_first) / B);
}

// grid: (rows + 1 over CSV_WG, slots).  seg_nulls[(segment * nslots + slot) * CSV_NULL_BANKS + bank], summed over the banks by the
// host, counts the NULLs a batch gets from this piece.
// Q (sqlrs_csv_set_device_quotes): a field that starts with '"' also ends in one — every quote of the rows is regular — and its
// value is what lies between them with "" read as '"'.  The host parser pops one '\r' from the end of a record's text at '\n'
// even when it came from inside the quotes: a closing quote directly in front of the record's '\n' drops a '\r' before it.
// A typed field with a quote left inside is an error (the host parser's to raise), as is a field the rule does not explain.
template <bool Q>
__global__ __launch_bounds__(CSV_WG) void csv_parse_kernel(const uint8_t *__restrict__ b, const uint32_t *__restrict__ sep_pos,
                                                           const CsvParams P, uint32_t *__restrict__ seg_nulls,
                                                           CsvPatch *__restrict__ patches, CsvCtl *__restrict__ ctl) {
  const int64_t row = (int64_t)blockIdx.x * CSV_WG + threadIdx.x;
  const int s = blockIdx.y;
  const CsvSlot &S = P.slot[s];
  const bool utf8 = S.dtype == SQLRS_UTF8;
  if (row == P.rows && utf8) S.ulen[row] = 0;
  const bool live = row < P.rows;
  bool null_row = false;
  if (live) {
    const int64_t f = row * P.C + S.src;
    uint32_t start = f == 0 ? 0u : sep_pos[f - 1] + 1, end = sep_pos[f];
    if (S.src == 0) // blank lines in front of the record ('\n' or "\r\n" straight after a record's end)
      while (start < end) {
        if (b[start] == '\n') start++;
        else if (b[start] == '\r' && b[start + 1] == '\n') start += 2;
        else break;
      }
    if (S.src == P.C - 1 && end > start && b[end - 1] == '\r') end--; // one trailing '\r' of the record
    uint32_t inner_quotes = 0;
    bool quote_error = false;
    if (Q && end > start && b[start] == '"') {
      if (end - start < 2 || b[end - 1] != '"') quote_error = true;
      else {
        const bool at_newline = b[end] == '\n';
        start++;
        end--;
        if (at_newline && end > start && b[end - 1] == '\r') end--;
        for (uint32_t k = start; k < end; k++) inner_quotes += b[k] == '"';
        quote_error = (inner_quotes & 1) != 0;
      }
    }
    if (utf8) {
      if (quote_error) atomicMin(&ctl->err_row, (uint32_t)row);
      S.ustart[row] = start | (inner_quotes ? CSV_ESCAPES : 0u);
      S.ulen[row] = quote_error ? 0u : end - start - inner_quotes / 2;
    } else {
      uint64_t v = 0;
      int res = CSV_FIELD_OK;
      null_row = start == end;
      if (quote_error || inner_quotes) res = CSV_FIELD_ERROR;
      else if (!null_row) {
        if (S.dtype == SQLRS_INT64) res = csv_parse_int64(b + start, b + end, v);
        else if (S.dtype == SQLRS_FLOAT64) res = csv_parse_float64(b + start, b + end, v);
        else res = csv_parse_bool(b + start, b + end, v);
      }
      if (res == CSV_FIELD_ERROR) atomicMin(&ctl->err_row, (uint32_t)row);
      else if (res == CSV_FIELD_PATCH) patches[atomicAdd(&ctl->num_patches, 1u)] = CsvPatch{(uint32_t)row, (uint32_t)s, start, end - start};
      S.val[row] = v;
      S.flag[row] = null_row ? 0 : 1;
    }
  }
  // NULLs per output batch: the workgroup's 256 rows lie in one segment almost always — one atomic for the workgroup, on one
  // of CSV_NULL_BANKS counters (with 2^22-row batches every workgroup of a piece adds to the same (segment, slot))
  __shared__ uint32_t s_nulls;
  if (threadIdx.x == 0) s_nulls = 0;
  __syncthreads();
  const uint64_t nulls = __ballot(null_row);
  const int64_t row0 = (int64_t)blockIdx.x * CSV_WG;
  const uint32_t seg_lo = csv_segment(row0, P.seg_first, P.B), seg_hi = csv_segment(min(row0 + CSV_WG - 1, P.rows - 1), P.seg_first, P.B);
  const uint32_t bank = blockIdx.x % CSV_NULL_BANKS;
  if (seg_lo == seg_hi) {
    if (nulls && lane_id() == 0) atomicAdd(&s_nulls, (uint32_t)__popcll(nulls));
    __syncthreads();
    if (threadIdx.x == 0 && s_nulls) atomicAdd(&seg_nulls[((size_t)seg_lo * P.nslots + s) * CSV_NULL_BANKS + bank], s_nulls);
  } else if (null_row)
    atomicAdd(&seg_nulls[((size_t)csv_segment(row, P.seg_first, P.B) * P.nslots + s) * CSV_NULL_BANKS + bank], 1u);
}

// Utf8 bytes per (segment, slot) out of the scanned lengths; grid over segments, slots in y
__global__ void csv_seg_bytes_kernel(const CsvParams P, int64_t nseg, uint32_t *__restrict__ seg_bytes) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int s = blockIdx.y;
  if (g >= nseg || P.slot[s].dtype != SQLRS_UTF8) return;
  const int64_t lo = g == 0 ? 0 : min(P.rows, P.seg_first + (g - 1) * P.B), hi = min(P.rows, P.seg_first + g * P.B);
  seg_bytes[(size_t)g * P.nslots + s] = P.slot[s].uoff[hi] - P.slot[s].uoff[lo];
}

// the values std::from_chars gave the patch list's fields
__global__ void csv_patch_kernel(const CsvParams P, const CsvPatch *__restrict__ patches, const uint64_t *__restrict__ vals, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) P.slot[patches[i].slot].val[patches[i].row] = vals[i];
}

// rows [a, a + cnt) of the piece -> rows [fill, fill + cnt) of the batch under construction; grid: (cnt over CSV_WG, slots)
// Q: a Utf8 field marked CSV_ESCAPES is copied without the second quote of each "" pair
template <bool Q>
__global__ __launch_bounds__(CSV_WG) void csv_cut_kernel(const uint8_t *__restrict__ b, const CsvParams P, const CsvOutParams O,
                                                         int64_t a, int64_t cnt, int64_t fill) {
  const int64_t i = (int64_t)blockIdx.x * CSV_WG + threadIdx.x;
  if (i >= cnt) return;
  const CsvSlot &S = P.slot[blockIdx.y];
  const CsvOut &D = O.out[blockIdx.y];
  if (S.dtype == SQLRS_UTF8) {
    const uint32_t o0 = S.uoff[a], o = S.uoff[a + i], len = S.ulen[a + i];
    const uint32_t dst = D.ubase + (o - o0);
    if (i == 0) D.offsets[fill] = (int32_t)D.ubase;
    D.offsets[fill + i + 1] = (int32_t)(dst + len);
    const uint32_t st = S.ustart[a + i];
    if (Q && (st & CSV_ESCAPES)) {
      const uint8_t *src = b + (st & ~CSV_ESCAPES);
      for (uint32_t k = 0; k < len; k++) {
        const uint8_t c = *src;
        D.bytes[dst + k] = c;
        src += c == '"' ? 2 : 1;
      }
    } else {
      const uint8_t *src = b + st;
      for (uint32_t k = 0; k < len; k++) D.bytes[dst + k] = src[k];
    }
  } else {
    const uint64_t v = S.val[a + i];
    const uint8_t ok = S.flag[a + i];
    if (S.dtype == SQLRS_BOOLEAN) D.vb[fill + i] = (uint8_t)(ok | (v ? 2 : 0));
    else {
      D.values[fill + i] = v;
      D.vb[fill + i] = ok;
    }
  }
}

// a finished batch's flag bytes -> bitmaps, one ballot word per wave; grid: (rows over CSV_WG, slots)
__global__ __launch_bounds__(CSV_WG) void csv_pack_kernel(const CsvParams P, const CsvOutParams O, int64_t rows) {
  const int64_t i = (int64_t)blockIdx.x * CSV_WG + threadIdx.x;
  const int32_t dtype = P.slot[blockIdx.y].dtype;
  if (dtype == SQLRS_UTF8) return;
  const CsvOut &D = O.out[blockIdx.y];
  const uint8_t f = i < rows ? D.vb[i] : 0;
  const uint64_t valid = __ballot(f & 1), truth = __ballot(f & 2);
  if (lane_id() == 0 && i < rows) {
    D.validity[i >> 6] = valid;
    if (dtype == SQLRS_BOOLEAN) D.values[i >> 6] = truth;
  }
}

} // namespace sq
