// csv_device.hip — the CSV reader's device parser (sqlrs_csv_set_device_parse): the file is read in pieces into pinned
// memory, a piece is cut at its last '\n', uploaded and taken apart by the kernels of csv_kernels.hpp; sqlrs_csv_next_batch
// hands out batch_size rows at a time, cut from what the pieces produced (a batch may span pieces, a piece many batches).
//
// The host parser (plumbing.hip) is the specification, and the fallback at two granularities:
//   * a piece with a '"' byte (sqlrs_csv_set_device_quotes: a piece with an irregular quote in front of its last record
//     end), a record longer than a piece, and the batch in which the device found an error are read by the host parser:
//     the file is positioned at the first record of the batch under construction and whole batches are parsed there
//     until the file position is behind the piece (an error: the host parser raises its own message, and the reader
//     stays with it) — the stream of batches is the host parser's by construction;
//   * a Float64 field outside csv_parse_float64's exactly rounded rule is written by std::from_chars (the patch list).
// With sqlrs_csv_set_device_quotes a piece is cut at its last '\n' outside quotes, which the device reports.
// Two host round trips per piece: (separators, first ragged row, quote flag / first irregular quote and the cut), then
// (error row, patch list, NULLs and Utf8 bytes per output batch, where the trailing batch starts); none per batch.
#include <algorithm>
#include <charconv>

#include "csv_kernels.hpp"
#include "csv_reader.hpp"
#include "prims.hpp"

namespace sq {

constexpr int64_t CSV_DEFAULT_PIECE = 32ll << 20;
constexpr int64_t CSV_MAX_PIECE = 0x7fffffffll - 64; // Utf8 offsets are int32, row ids and byte positions 32-bit

struct CsvDevice {
  int64_t piece_bytes = CSV_DEFAULT_PIECE;
  int64_t device_rows = 0, host_rows = 0, patched = 0;
  bool started = false, host_forever = false;
  int64_t pos = 0, file_size = 0; // the next piece starts here (always the first byte after a record's end)
  int64_t host_until = -1;        // >= 0: the host parser reads until the file position is here or behind it
  uint8_t *pin = nullptr;         // the piece's bytes
  uint8_t *ctl_pin = nullptr;     // control words up, counts and lists down
  size_t ctl_cap = 0;
  // ---- the piece in HBM
  BufP bytes, sep_pos, tile_cnt, tile_off, tile_quotes, tile_qoff, total, ctl, seg_stats, patches, patch_vals, vb;
  struct Slot {
    BufP val, flag, ustart, ulen, uoff;
  };
  std::vector<Slot> slots;
  CsvParams P;
  int64_t piece_pos = 0, piece_rows = 0, piece_next = 0, nseg = 0, tail_start_off = 0;
  bool piece_trouble = false; // the row behind piece_rows is one the host parser has to look at
  bool piece_quotes = false;  // parsed by the quote-aware kernels
  std::vector<uint32_t> seg_nulls, seg_bytes;
  // ---- the batch under construction
  struct Col {
    BufP values, validity, offsets, bytes;
    int64_t nulls = 0, ubytes = 0;
  };
  std::vector<Col> pend;
  int64_t fill = 0, cap = 0;
  int64_t pend_start_row = -1; // its first row in the current piece (-1: it began in an earlier piece, at batch_start_off)
  int64_t batch_start_off = 0;
  uint64_t batch_start_line = 0;
  ~CsvDevice() {
    if (pin) (void)hipHostFree(pin);
    if (ctl_pin) (void)hipHostFree(ctl_pin);
  }
};

namespace {

void need(Ctx *ctx, BufP &b, size_t bytes) {
  if (!b || b->cap < bytes) b = ctx->alloc(bytes);
}
void need_ctl(Ctx *ctx, CsvDevice &d, size_t bytes) {
  if (bytes <= d.ctl_cap) return;
  ctx->sync(); // (copies out of the old block may be in flight)
  const size_t cap = std::max(bytes, 2 * d.ctl_cap);
  uint8_t *p = nullptr;
  SQ_HIP(hipHostMalloc((void **)&p, cap, hipHostMallocDefault));
  if (d.ctl_pin) {
    std::memcpy(p, d.ctl_pin, d.ctl_cap);
    (void)hipHostFree(d.ctl_pin);
  }
  d.ctl_pin = p;
  d.ctl_cap = cap;
}
constexpr size_t CTL_DOWN = 64; // ctl_pin: [0, 64) goes up, the rest comes down

int64_t row_start(sqlrs_csv *r, CsvDevice &d, int64_t row) { // file offset of a row of the current piece
  if (row == 0) return d.piece_pos;
  const uint32_t *p = d.sep_pos->as<uint32_t>() + row * (int64_t)r->names.size() - 1;
  return d.piece_pos + (int64_t)r->ctx->fetch_value(p) + 1;
}

// The host parser takes over at the first record of the batch under construction (`off` when there is none); what the
// device had put into that batch is dropped.
void rewind_to_host(sqlrs_csv *r, CsvDevice &d, int64_t off, int64_t until) {
  if (d.fill > 0) {
    off = d.pend_start_row >= 0 ? row_start(r, d, d.pend_start_row) : d.batch_start_off;
    r->line = d.batch_start_line;
    if (r->remaining != ~0ull) r->remaining += (uint64_t)d.fill;
  }
  d.pend.clear();
  d.fill = 0;
  d.pend_start_row = -1;
  d.piece_rows = d.piece_next = 0;
  d.piece_trouble = false;
  r->file.clear();
  r->file.seekg(off);
  if (until < 0) d.host_forever = true;
  else d.host_until = until;
}

CsvOutParams out_params(sqlrs_csv *r, CsvDevice &d) {
  CsvOutParams O;
  std::memset(&O, 0, sizeof(O));
  for (size_t s = 0; s < d.pend.size(); s++) {
    CsvDevice::Col &c = d.pend[s];
    CsvOut &o = O.out[s];
    o.values = c.values ? c.values->as<uint64_t>() : nullptr;
    o.validity = c.validity ? c.validity->as<uint64_t>() : nullptr;
    o.offsets = c.offsets ? c.offsets->as<int32_t>() : nullptr;
    o.bytes = c.bytes ? c.bytes->as<uint8_t>() : nullptr;
    o.vb = d.vb->as<uint8_t>() + s * (size_t)r->batch_size;
    o.ubase = (uint32_t)c.ubytes;
  }
  return O;
}

// reads, uploads and parses the piece at d.pos; leaves piece_rows good rows to cut batches from, or hands over to the host
void load_piece(sqlrs_csv *r, CsvDevice &d) {
  Ctx *ctx = r->ctx;
  const int64_t C = (int64_t)r->names.size(), B = r->batch_size;
  const int nslots = (int)r->projection.size();
  if (!d.pin) SQ_HIP(hipHostMalloc((void **)&d.pin, (size_t)d.piece_bytes + 16, hipHostMallocDefault));
  need_ctl(ctx, d, 4096);
  r->file.clear();
  r->file.seekg(d.pos);
  r->file.read((char *)d.pin, d.piece_bytes);
  const int64_t n = (int64_t)r->file.gcount();
  r->file.clear();
  d.piece_pos = d.pos;
  d.piece_rows = d.piece_next = 0;
  d.piece_trouble = false;
  if (n <= 0) {
    d.pos = d.file_size = d.piece_pos; // (the file ends here)
    return;
  }
  const bool last = d.pos + n >= d.file_size;
  int64_t len = n, consumed = n;
  if (last) {
    if (d.pin[n - 1] != '\n') d.pin[len++] = '\n'; // a last record without '\n' counts
  } else {
    const void *q = memrchr(d.pin, '\n', (size_t)n);
    if (!q) return rewind_to_host(r, d, d.piece_pos, d.piece_pos + n); // a record longer than a piece
    len = consumed = (const uint8_t *)q - d.pin + 1;                    // the cut record is the next piece's first
  }
  // ---- classify, rank and check the separators
  const int64_t ntiles = ceil_div(len, CSV_TILE);
  need(ctx, d.bytes, round_up((size_t)len, 16) + 16);
  need(ctx, d.sep_pos, 4 * (size_t)len + 16);
  need(ctx, d.tile_cnt, 4 * (size_t)ntiles);
  need(ctx, d.tile_off, 4 * (size_t)ntiles);
  need(ctx, d.total, 8);
  need(ctx, d.ctl, sizeof(CsvCtl));
  const uint8_t *bytes = d.bytes->as<uint8_t>();
  CsvCtl *ctl = d.ctl->as<CsvCtl>();
  *(CsvCtl *)d.ctl_pin = CsvCtl{0, CSV_NO_ROW, CSV_NO_ROW, 0, CSV_NO_ROW, 0, 0, 0};
  // (a delimiter that is a quote or a line end's byte: the quote rule is not stated for it)
  const bool Q = d.piece_quotes = r->device_quotes && r->delimiter != '"' && r->delimiter != '\n' && r->delimiter != '\r';
  SQ_HIP(hipMemcpyAsync(d.bytes->p, d.pin, (size_t)len, hipMemcpyHostToDevice, ctx->stream));
  SQ_HIP(hipMemcpyAsync(ctl, d.ctl_pin, sizeof(CsvCtl), hipMemcpyHostToDevice, ctx->stream));
  if (Q) { // the parity pass runs whether the piece has quotes or not: no round trip to find out
    need(ctx, d.tile_quotes, 4 * (size_t)ntiles);
    need(ctx, d.tile_qoff, 4 * (size_t)ntiles);
    const uint32_t *qoff = d.tile_qoff->as<uint32_t>();
    {
      ProfScope ps(ctx, "csv_quotes");
      csv_quotes_kernel<<<dim3((unsigned)ntiles), dim3(CSV_WG), 0, ctx->stream>>>(bytes, len, d.tile_quotes->as<uint32_t>());
    }
    exclusive_scan_u32(ctx, d.tile_quotes->as<uint32_t>(), ntiles, nullptr, d.tile_qoff->as<uint32_t>(), d.total->as<uint64_t>());
    {
      ProfScope ps(ctx, "csv_classify_q");
      csv_classify_q_kernel<<<dim3((unsigned)ntiles), dim3(CSV_WG), 0, ctx->stream>>>(bytes, len, (uint8_t)r->delimiter, qoff,
                                                                                     d.tile_cnt->as<uint32_t>());
    }
    exclusive_scan_u32(ctx, d.tile_cnt->as<uint32_t>(), ntiles, nullptr, d.tile_off->as<uint32_t>(), d.total->as<uint64_t>());
    {
      ProfScope ps(ctx, "csv_index_q");
      csv_index_q_kernel<<<dim3((unsigned)ntiles), dim3(CSV_WG), 0, ctx->stream>>>(
          bytes, len, (uint8_t)r->delimiter, (uint32_t)C, qoff, d.tile_off->as<uint32_t>(), d.sep_pos->as<uint32_t>(), ctl);
    }
  } else {
    {
      ProfScope ps(ctx, "csv_classify");
      csv_classify_kernel<<<dim3((unsigned)ntiles), dim3(CSV_WG), 0, ctx->stream>>>(bytes, len, (uint8_t)r->delimiter,
                                                                                   d.tile_cnt->as<uint32_t>(), ctl);
    }
    exclusive_scan_u32(ctx, d.tile_cnt->as<uint32_t>(), ntiles, nullptr, d.tile_off->as<uint32_t>(), d.total->as<uint64_t>());
    {
      ProfScope ps(ctx, "csv_index");
      csv_index_kernel<<<dim3((unsigned)ntiles), dim3(CSV_WG), 0, ctx->stream>>>(bytes, len, (uint8_t)r->delimiter, (uint32_t)C,
                                                                                d.tile_off->as<uint32_t>(), d.sep_pos->as<uint32_t>(), ctl);
    }
  }
  SQ_HIP(hipGetLastError());
  uint8_t *down = d.ctl_pin + CTL_DOWN;
  SQ_HIP(hipMemcpyAsync(down, ctl, sizeof(CsvCtl), hipMemcpyDeviceToHost, ctx->stream));
  SQ_HIP(hipMemcpyAsync(down + 32, d.total->p, 8, hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  CsvCtl c = *(const CsvCtl *)down;
  uint64_t nsep = *(const uint64_t *)(down + 32);
  if (c.quote) return rewind_to_host(r, d, d.piece_pos, d.piece_pos + consumed);
  if (Q) {
    // the cut: the last record end outside quotes.  None: a record longer than the piece.  What lies behind it is the next
    // piece's, its separators (ranks >= nsep) and quotes included
    if (c.last_end_pos == 0) return rewind_to_host(r, d, d.piece_pos, d.piece_pos + n);
    consumed = std::min(n, (int64_t)c.last_end_pos + 1);
    if (c.bad_quote < c.last_end_pos) return rewind_to_host(r, d, d.piece_pos, d.piece_pos + consumed);
    nsep = (uint64_t)c.last_end_rank + 1;
    if (c.first_bad != CSV_NO_ROW && (uint64_t)c.first_bad * (uint64_t)C >= nsep) c.first_bad = CSV_NO_ROW;
  }
  int64_t R = c.first_bad != CSV_NO_ROW ? (int64_t)c.first_bad : (int64_t)(nsep / (uint64_t)C);
  bool trouble = c.first_bad != CSV_NO_ROW;
  if ((uint64_t)R >= r->remaining) { // the bounds end the scan before the ragged record is read
    R = (int64_t)r->remaining;
    trouble = false;
  }
  d.pos = d.piece_pos + consumed;
  if (R > 0) {
    // ---- parse rows [0, R): rows [0, seg_first) finish the batch under construction, then batches of B rows
    CsvParams &P = d.P;
    std::memset(&P, 0, sizeof(P));
    P.nslots = nslots;
    P.C = (int)C;
    P.rows = R;
    P.seg_first = std::min(R, B - d.fill);
    P.B = B;
    d.nseg = 1 + ceil_div(R - P.seg_first, B);
    d.slots.resize((size_t)nslots);
    int nfloat = 0, nutf8 = 0;
    for (int s = 0; s < nslots; s++) {
      CsvDevice::Slot &S = d.slots[(size_t)s];
      CsvSlot &ps = P.slot[s];
      ps.src = r->projection[(size_t)s];
      ps.dtype = r->dtypes[(size_t)ps.src];
      if (ps.dtype == SQLRS_UTF8) {
        need(ctx, S.ustart, 4 * (size_t)R);
        need(ctx, S.ulen, 4 * (size_t)(R + 1));
        need(ctx, S.uoff, 4 * (size_t)(R + 1));
        ps.ustart = S.ustart->as<uint32_t>();
        ps.ulen = S.ulen->as<uint32_t>();
        ps.uoff = S.uoff->as<uint32_t>();
        nutf8++;
      } else {
        need(ctx, S.val, 8 * (size_t)R);
        need(ctx, S.flag, (size_t)R);
        ps.val = S.val->as<uint64_t>();
        ps.flag = S.flag->as<uint8_t>();
        nfloat += ps.dtype == SQLRS_FLOAT64;
      }
    }
    const size_t nstat = (size_t)d.nseg * (size_t)nslots;
    const size_t nstat_dev = nstat * (CSV_NULL_BANKS + 1); // NULL counters in banks, then the Utf8 bytes
    d.seg_stats = ctx->alloc_zero(4 * nstat_dev);
    uint32_t *seg_nulls = d.seg_stats->as<uint32_t>(), *seg_bytes = seg_nulls + nstat * CSV_NULL_BANKS;
    if (nfloat) need(ctx, d.patches, sizeof(CsvPatch) * (size_t)R * (size_t)nfloat);
    {
      ProfScope ps(ctx, "csv_parse");
      const dim3 grid((unsigned)ceil_div(R + 1, CSV_WG), (unsigned)nslots);
      CsvPatch *patches = nfloat ? d.patches->as<CsvPatch>() : nullptr;
      if (Q) csv_parse_kernel<true><<<grid, dim3(CSV_WG), 0, ctx->stream>>>(bytes, d.sep_pos->as<uint32_t>(), P, seg_nulls, patches, ctl);
      else csv_parse_kernel<false><<<grid, dim3(CSV_WG), 0, ctx->stream>>>(bytes, d.sep_pos->as<uint32_t>(), P, seg_nulls, patches, ctl);
    }
    for (int s = 0; s < nslots; s++)
      if (P.slot[s].dtype == SQLRS_UTF8)
        exclusive_scan_u32(ctx, P.slot[s].ulen, R + 1, nullptr, d.slots[(size_t)s].uoff->as<uint32_t>(), d.total->as<uint64_t>());
    if (nutf8) {
      ProfScope ps(ctx, "csv_seg_bytes");
      csv_seg_bytes_kernel<<<dim3((unsigned)ceil_div(d.nseg, 256), (unsigned)nslots), dim3(256), 0, ctx->stream>>>(P, d.nseg, seg_bytes);
    }
    SQ_HIP(hipGetLastError());
    need_ctl(ctx, d, CTL_DOWN + 48 + 4 * nstat_dev);
    down = d.ctl_pin + CTL_DOWN;
    SQ_HIP(hipMemcpyAsync(down, ctl, sizeof(CsvCtl), hipMemcpyDeviceToHost, ctx->stream));
    const int64_t a_last = d.nseg > 1 ? P.seg_first + (d.nseg - 2) * B : 0; // where the piece's last batch starts
    if (a_last > 0)
      SQ_HIP(hipMemcpyAsync(down + 32, d.sep_pos->as<uint32_t>() + a_last * C - 1, 4, hipMemcpyDeviceToHost, ctx->stream));
    SQ_HIP(hipMemcpyAsync(down + 48, seg_nulls, 4 * nstat_dev, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    c = *(const CsvCtl *)down;
    d.tail_start_off = a_last > 0 ? d.piece_pos + (int64_t)*(const uint32_t *)(down + 32) + 1 : d.piece_pos;
    const uint32_t *st = (const uint32_t *)(down + 48);
    d.seg_nulls.assign(nstat, 0);
    for (size_t i = 0; i < nstat * CSV_NULL_BANKS; i++) d.seg_nulls[i / CSV_NULL_BANKS] += st[i];
    d.seg_bytes.assign(st + nstat * CSV_NULL_BANKS, st + nstat_dev);
    int64_t err_row = c.err_row != CSV_NO_ROW ? (int64_t)c.err_row : R;
    if (c.num_patches) { // the fields the device left to std::from_chars
      const size_t np = c.num_patches;
      need_ctl(ctx, d, CTL_DOWN + 24 * np);
      CsvPatch *pl = (CsvPatch *)(d.ctl_pin + CTL_DOWN);
      uint64_t *vals = (uint64_t *)(d.ctl_pin + CTL_DOWN + 16 * np);
      SQ_HIP(hipMemcpyAsync(pl, d.patches->p, 16 * np, hipMemcpyDeviceToHost, ctx->stream));
      ctx->sync();
      for (size_t i = 0; i < np; i++) {
        const char *p = (const char *)d.pin + pl[i].start;
        double v = 0;
        auto pr = std::from_chars(p, p + pl[i].len, v);
        if (pr.ec != std::errc() || pr.ptr != p + pl[i].len) err_row = std::min(err_row, (int64_t)pl[i].row);
        std::memcpy(&vals[i], &v, 8);
      }
      need(ctx, d.patch_vals, 8 * np);
      SQ_HIP(hipMemcpyAsync(d.patch_vals->p, vals, 8 * np, hipMemcpyHostToDevice, ctx->stream));
      ProfScope ps(ctx, "csv_patch");
      csv_patch_kernel<<<dim3((unsigned)ceil_div((int64_t)np, 256)), dim3(256), 0, ctx->stream>>>(
          P, d.patches->as<CsvPatch>(), d.patch_vals->as<uint64_t>(), (uint32_t)np);
      SQ_HIP(hipGetLastError());
      d.patched += (int64_t)np;
    }
    if (err_row < R) {
      R = err_row;
      trouble = true;
    }
  }
  d.piece_rows = R;
  d.piece_trouble = trouble;
}

// the next segment of the piece -> the batch under construction
void append_segment(sqlrs_csv *r, CsvDevice &d) {
  Ctx *ctx = r->ctx;
  const int64_t B = r->batch_size, a = d.piece_next;
  const int nslots = (int)r->projection.size();
  const int64_t take = std::min(d.piece_rows - a, B - d.fill);
  const size_t seg = a < d.P.seg_first ? 0 : 1 + (size_t)((a - d.P.seg_first) / B);
  if (d.fill == 0) { // a new batch
    d.cap = r->remaining != ~0ull ? (int64_t)std::min<uint64_t>((uint64_t)B, r->remaining) : B;
    d.pend.assign((size_t)nslots, CsvDevice::Col());
    for (int s = 0; s < nslots; s++) {
      CsvDevice::Col &c = d.pend[(size_t)s];
      const int32_t dt = d.P.slot[s].dtype;
      if (dt == SQLRS_UTF8) c.offsets = ctx->alloc(4 * (size_t)(d.cap + 1));
      else {
        c.values = ctx->alloc(dt == SQLRS_BOOLEAN ? bitmap_bytes(d.cap) : 8 * (size_t)d.cap);
        c.validity = ctx->alloc(bitmap_bytes(d.cap));
      }
    }
    need(ctx, d.vb, (size_t)nslots * (size_t)B);
    d.pend_start_row = a;
    d.batch_start_line = r->line;
  }
  for (int s = 0; s < nslots; s++) {
    if (d.P.slot[s].dtype != SQLRS_UTF8) continue;
    CsvDevice::Col &c = d.pend[(size_t)s];
    const size_t want = (size_t)c.ubytes + d.seg_bytes[seg * (size_t)nslots + (size_t)s];
    if (want > 0x7fffffffull) fail(SQLRS_ERR_ARROW, "csv: a Utf8 column of one batch overflows int32 offsets");
    if (!c.bytes || c.bytes->cap < want) {
      BufP nb = ctx->alloc(std::max(want, c.bytes ? 2 * c.bytes->cap : (size_t)0));
      if (c.ubytes) SQ_HIP(hipMemcpyAsync(nb->p, c.bytes->p, (size_t)c.ubytes, hipMemcpyDeviceToDevice, ctx->stream));
      c.bytes = nb;
    }
  }
  {
    ProfScope ps(ctx, "csv_cut");
    const dim3 grid((unsigned)ceil_div(take, CSV_WG), (unsigned)nslots);
    if (d.piece_quotes) csv_cut_kernel<true><<<grid, dim3(CSV_WG), 0, ctx->stream>>>(d.bytes->as<uint8_t>(), d.P, out_params(r, d), a, take, d.fill);
    else csv_cut_kernel<false><<<grid, dim3(CSV_WG), 0, ctx->stream>>>(d.bytes->as<uint8_t>(), d.P, out_params(r, d), a, take, d.fill);
    SQ_HIP(hipGetLastError());
  }
  for (int s = 0; s < nslots; s++) {
    d.pend[(size_t)s].nulls += d.seg_nulls[seg * (size_t)nslots + (size_t)s];
    d.pend[(size_t)s].ubytes += d.seg_bytes[seg * (size_t)nslots + (size_t)s];
  }
  d.fill += take;
  d.piece_next += take;
  r->line += (uint64_t)take;
  if (r->remaining != ~0ull) r->remaining -= (uint64_t)take;
}

void emit_pending(sqlrs_csv *r, CsvDevice &d, int out_mem, sqlrs_batch_t **out) {
  Ctx *ctx = r->ctx;
  const int nslots = (int)r->projection.size();
  const int64_t rows = d.fill;
  {
    ProfScope ps(ctx, "csv_pack");
    csv_pack_kernel<<<dim3((unsigned)ceil_div(rows, CSV_WG), (unsigned)nslots), dim3(CSV_WG), 0, ctx->stream>>>(d.P, out_params(r, d), rows);
    SQ_HIP(hipGetLastError());
  }
  DBatch o;
  o.rows = rows;
  for (int s = 0; s < nslots; s++) {
    CsvDevice::Col &c = d.pend[(size_t)s];
    DCol col;
    col.dtype = d.P.slot[s].dtype;
    col.length = rows;
    col.null_count = c.nulls;
    if (col.dtype == SQLRS_UTF8) {
      if (!c.bytes) c.bytes = ctx->alloc(8);
      col.own_values = c.bytes;
      col.own_offsets = c.offsets;
      col.offsets = c.offsets->as<int32_t>();
      col.data_bytes = c.ubytes;
    } else {
      col.own_values = c.values;
      col.own_validity = c.validity;
      col.validity = c.validity->as<uint64_t>();
    }
    col.values = col.own_values->p;
    o.cols.push_back(std::move(col));
  }
  d.pend.clear();
  d.fill = 0;
  d.pend_start_row = -1;
  *out = emit_batch(ctx, std::move(o), out_mem);
  d.device_rows += rows;
}

} // namespace

void csv_device_next_batch(sqlrs_csv *r, int out_mem, sqlrs_batch_t **out) {
  Ctx *ctx = r->ctx;
  CsvDevice &d = *r->dev;
  *out = nullptr;
  if (out_mem != SQLRS_MEM_HOST && out_mem != SQLRS_MEM_DEVICE) fail(SQLRS_ERR_INTERNAL, "bad out_mem");
  SQ_HIP(hipSetDevice(ctx->device));
  if (!d.started) {
    d.started = true;
    r->file.clear();
    d.pos = (int64_t)r->file.tellg();
    r->file.seekg(0, std::ios::end);
    d.file_size = (int64_t)r->file.tellg();
    r->file.seekg(d.pos);
    const size_t nslots = r->projection.size();
    if (d.pos < 0 || nslots == 0 || nslots > (size_t)CSV_MAX_SLOTS) d.host_forever = true; // (a shape the kernels do not take)
  }
  for (;;) {
    if (d.host_forever || d.host_until >= 0) {
      try {
        csv_host_next_batch(r, out_mem, out);
      } catch (...) {
        d.host_forever = true; // (the host parser goes on behind the bad record, as it does on its own)
        throw;
      }
      if (*out) d.host_rows += (*out)->num_rows;
      if (*out && !d.host_forever) {
        const int64_t p = r->file.good() ? (int64_t)r->file.tellg() : -1;
        if (p < 0) d.host_forever = true; // the end of the file: the next call reports it
        else if (p >= d.host_until) {      // behind the piece, at a batch boundary: the device goes on from here
          d.pos = p;
          d.host_until = -1;
        }
      }
      return;
    }
    if (d.piece_next < d.piece_rows) {
      append_segment(r, d);
      if (d.fill == r->batch_size) return emit_pending(r, d, out_mem, out);
      continue;
    }
    if (d.piece_trouble) { // the record behind the good rows is the host parser's: it raises the error
      rewind_to_host(r, d, row_start(r, d, d.piece_rows), -1);
      continue;
    }
    if (d.fill > 0 && d.pend_start_row >= 0) { // the batch under construction leaves the piece it began in
      d.batch_start_off = d.pend_start_row == 0 ? d.piece_pos : d.tail_start_off;
      d.pend_start_row = -1;
    }
    d.piece_rows = d.piece_next = 0;
    if (r->remaining == 0 || d.pos >= d.file_size) { // the end of the scan
      if (d.fill > 0) emit_pending(r, d, out_mem, out);
      return;
    }
    load_piece(r, d);
  }
}

} // namespace sq

extern "C" {

int sqlrs_csv_set_device_parse(sqlrs_csv_t *r, int64_t chunk_bytes) {
  return sq::guard(r->ctx, [&] {
    if (r->dev && r->dev->started) sq::fail(SQLRS_ERR_INTERNAL, "sqlrs_csv_set_device_parse: after the first sqlrs_csv_next_batch");
    r->dev.reset();
    if (chunk_bytes == 0) return;
    r->dev = std::make_shared<sq::CsvDevice>();
    r->dev->piece_bytes = chunk_bytes < 0 ? sq::CSV_DEFAULT_PIECE : std::min(chunk_bytes, sq::CSV_MAX_PIECE);
  });
}

int sqlrs_csv_set_device_quotes(sqlrs_csv_t *r, int on) {
  return sq::guard(r->ctx, [&] {
    if (r->started) sq::fail(SQLRS_ERR_INTERNAL, "sqlrs_csv_set_device_quotes: after the first sqlrs_csv_next_batch");
    r->device_quotes = on != 0;
  });
}

int sqlrs_csv_device_stats(const sqlrs_csv_t *r, int64_t *device_rows, int64_t *host_rows, int64_t *patched_fields) {
  const sq::CsvDevice *d = r->dev.get();
  if (device_rows) *device_rows = d ? d->device_rows : 0;
  if (host_rows) *host_rows = d ? d->host_rows : 0;
  if (patched_fields) *patched_fields = d ? d->patched : 0;
  return SQLRS_OK;
}

} // extern "C"
