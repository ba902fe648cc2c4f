// dse_finish_host.cpp -- the finish side of the C-ABI host layer (include/dse.h):
// primes{k}.txt written by the host from a mask (dse_write_*_file), or formatted
// on the device (dse_finish.hip) from a mask that stays in HBM (dse_finish_*).
#include <algorithm>
#include <cstdio>

#include "dse_finish_fmt.h"
#include "dse_host.h"

using namespace dse;

// ---------------------------------------------------------------------------
// finish writer (sieve.clj:82-108)
// ---------------------------------------------------------------------------
namespace {

inline int fmt_u64(uint64_t v, char* out) {
  char t[24];
  int n = 0;
  do {
    t[n++] = (char)('0' + v % 10);
    v /= 10;
  } while (v);
  for (int i = 0; i < n; ++i) out[i] = t[n - 1 - i];
  return n;
}

// java.lang.Double.toString of an integer-valued double 1 <= v < 2^53.
inline int fmt_java_double(uint64_t v, char* out) {
  if (v < 10000000ull) {
    int n = fmt_u64(v, out);
    out[n++] = '.';
    out[n++] = '0';
    return n;
  }
  char d[24];
  int len = fmt_u64(v, d);
  int sig = len;
  while (sig > 1 && d[sig - 1] == '0') --sig;
  int n = 0;
  out[n++] = d[0];
  out[n++] = '.';
  if (sig == 1) out[n++] = '0';
  for (int i = 1; i < sig; ++i) out[n++] = d[i];
  out[n++] = 'E';
  n += fmt_u64((uint64_t)(len - 1), out + n);
  return n;
}

}  // namespace

extern "C" int32_t dse_write_range_file(const char* path, int32_t my_num, uint64_t g_start, uint64_t nbits,
                                        const uint64_t* mask) {
  if (!path || !mask) return fail(DSE_EINVAL, "null path or mask");
  if (my_num < 1) return fail(DSE_EINVAL, "my_num must be >= 1");
  if (my_num == 1 && nbits < 4) return fail(DSE_EINVAL, "finish's 2/3/5/7 hack needs a chunk of >= 4 candidates");
  const uint64_t cs = nbits;
  FILE* f = std::fopen(path, "wb");
  if (!f) return fail(DSE_EIO, std::string("cannot open ") + path);
  std::vector<char> buf(1 << 20);
  size_t used = 0;
  int per_line = 0;
  const uint64_t base = g_start;
  auto emit = [&](uint64_t v) {
    if (used + 64 > buf.size()) {
      std::fwrite(buf.data(), 1, used, f);
      used = 0;
    }
    if (per_line) {
      buf[used++] = ',';
      buf[used++] = ' ';
    }
    used += (size_t)(my_num == 1 ? fmt_java_double(v, buf.data() + used) : fmt_u64(v, buf.data() + used));
    if (++per_line == 10) {
      buf[used++] = '\n';
      per_line = 0;
    }
  };
  const uint64_t words = (cs + 63) / 64;
  uint64_t j0 = 0;
  if (my_num == 1) {  // positions 0..3 become 2.0 3.0 5.0 7.0 (sieve.clj:93-96)
    emit(2);
    emit(3);
    emit(5);
    emit(7);
    j0 = 4;
  }
  for (uint64_t w = j0 / 64; w < words; ++w) {
    uint64_t v = mask[w];
    if (w == j0 / 64) v &= ~0ull << (j0 % 64);
    if (w == words - 1 && (cs & 63)) v &= (1ull << (cs & 63)) - 1;
    while (v) {
      const int b = __builtin_ctzll(v);
      v &= v - 1;
      emit(3 + 2 * (base + w * 64 + (uint64_t)b));
    }
  }
  if (per_line) buf[used++] = '\n';
  std::fwrite(buf.data(), 1, used, f);
  if (std::fclose(f) != 0) return fail(DSE_EIO, std::string("write failed: ") + path);
  return DSE_OK;
}

extern "C" int32_t dse_write_primes_file(const char* path, int32_t my_num, int64_t n, int32_t P,
                                         const uint64_t* mask) {
  int64_t cs;
  int32_t rc = chunk_geometry(n, P, &cs);
  if (rc) return rc;
  if (my_num < 1 || my_num > P) return fail(DSE_EINVAL, "my_num outside 1..P");
  if (cs < 4) return fail(DSE_EINVAL, "finish's 2/3/5/7 hack needs a chunk of >= 4 candidates");
  return dse_write_range_file(path, my_num, (uint64_t)(my_num - 1) * (uint64_t)cs, (uint64_t)cs, mask);
}

// ---------------------------------------------------------------------------
// finish on the device (dse_finish.hip): the mask stays in HBM, text comes back
// ---------------------------------------------------------------------------
namespace {

constexpr uint32_t kFinishFlagsAll = DSE_FINISH_DOUBLES | DSE_FINISH_HACK | DSE_FINISH_LAST;

// what both the async entry point and the file entry points refuse
int32_t finish_check_range(uint32_t flags, uint64_t g_start, uint64_t nbits) {
  if (flags & ~kFinishFlagsAll) return fail(DSE_EINVAL, "unknown finish flag");
  if ((flags & DSE_FINISH_HACK) && nbits < 4)
    return fail(DSE_EINVAL, "finish's 2/3/5/7 hack needs a chunk of >= 4 candidates");
  if (int32_t rc = check_odd_range(g_start, nbits)) return rc;  // bounds the next line's arithmetic
  if ((flags & DSE_FINISH_DOUBLES) && nbits && 3 + 2 * (g_start + nbits - 1) >= (1ull << 53))
    return fail(DSE_ERANGE, "Double printing needs every value below 2^53");
  return check_mask_range("finish", g_start, nbits);
}

// The three launches on `stream`, with the context's tile-sum scratch ordered
// against whatever stream used it last.
int32_t finish_launch(DevState& d, uint32_t flags, uint64_t g_start, uint64_t nbits, const uint64_t* mask_dev,
                      uint64_t first_rank, void* text_dev, uint64_t text_cap, unsigned long long* totals_dev,
                      hipStream_t stream) {
  return scratch_launch(d.finish_sums, finish_scratch_bytes(nbits), stream, "launch_finish_text", [&](void* sum) {
    return launch_finish_text(flags, g_start, nbits, mask_dev, first_rank, text_dev, text_cap, totals_dev, sum, stream);
  });
}

// The slab pipeline: mask_dev (ready in d.stream's order) -> file. Slab i+1 is
// formatted on d.stream while slab i's text is copied on the copy stream and
// slab i-1 is written to the file by this thread. The rank of a slab's first
// entry is the sum of the entry counts before it, so a slab is launched once
// the totals of the one before it are on the host.
int32_t finish_pipeline(dse_ctx* ctx, DevState& d, FILE* fp, const char* path, uint32_t flags, uint64_t g_start,
                        uint64_t nbits, const uint64_t* mask_dev, uint64_t* count_out) {
  const uint64_t words = (nbits + 63) / 64;
  if (count_out) *count_out = 0;
  if (!words) return DSE_OK;  // no entries: an empty file
  int32_t rc;
  if ((rc = ensure_slab_pipe(d, dse_finish_text_bound(g_start, nbits, nbits, flags)))) return rc;
  SlabPipe& f = d.pipe;
  const uint64_t B = f.buf_bytes;
  const uint64_t cap_words = ctx->finish_slab_words ? ctx->finish_slab_words : ~0ull;
  uint64_t rank = 0;

  auto launch = [&](int slot, uint64_t w0, uint64_t nw) -> int32_t {
    uint32_t fl = flags & DSE_FINISH_DOUBLES;
    if (w0 == 0) fl |= flags & DSE_FINISH_HACK;
    if (w0 + nw == words) fl |= DSE_FINISH_LAST;
    const uint64_t nb = std::min<uint64_t>(nbits - w0 * 64, nw * 64);
    int32_t r;
    if ((r = slab_reuse(f, slot, d.stream))) return r;
    if ((r = finish_launch(d, fl, g_start + w0 * 64, nb, mask_dev + w0, rank, f.dbuf[slot].ptr, B,
                           f.dtotals + 2 * slot, d.stream)))
      return r;
    HIP_TRY(hipMemcpyAsync(f.htotals + 2 * slot, f.dtotals + 2 * slot, 2 * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, d.stream));
    return DSE_OK;
  };
  auto write_slab = [&](int slot, uint64_t bytes) -> int32_t {  // once its copy has run
    if (int32_t r = slab_wait(f, slot)) return r;
    if (bytes && std::fwrite(f.hbuf[slot].ptr, 1, bytes, fp) != bytes)
      return fail(DSE_EIO, std::string("write failed: ") + path);
    return DSE_OK;
  };
  auto run = [&]() -> int32_t {
    int32_t r;
    int slot = 0, prev_slot = -1;
    uint64_t w0 = 0, prev_bytes = 0;
    // first guess: 128 text bytes per mask word (a prime mask prints 70..110); later slabs
    // are sized from the slab before them, and one that does not fit is halved and redone
    uint64_t nw = std::min(std::min(words, cap_words), std::max<uint64_t>(B / 128, 1));
    if ((r = launch(slot, w0, nw))) return r;
    for (;;) {
      HIP_TRY(hipStreamSynchronize(d.stream));  // the slab's launch is the stream's last work: its totals
      const uint64_t cnt = f.htotals[2 * slot], bytes = f.htotals[2 * slot + 1];
      if (bytes > B) {  // nothing was written: split the slab and format it again
        if (nw == 1) return fail(DSE_EINTERNAL, "finish: one mask word exceeds the text buffer");
        nw /= 2;
        if ((r = launch(slot, w0, nw))) return r;
        continue;
      }
      if ((r = slab_send(f, slot, bytes, d.stream))) return r;
      rank += cnt;
      const uint64_t w_next = w0 + nw;
      const bool more = w_next < words;
      uint64_t nw_next = 0;
      if (more) {
        const uint64_t per_word = bytes / nw + 1;
        nw_next = std::max<uint64_t>((B - B / 8) / per_word, 1);
        nw_next = std::min(std::min(nw_next, words - w_next), cap_words);
        if ((r = launch(slot ^ 1, w_next, nw_next))) return r;
      }
      if (prev_slot >= 0 && (r = write_slab(prev_slot, prev_bytes))) return r;
      prev_slot = slot;
      prev_bytes = bytes;
      if (!more) break;
      slot ^= 1;
      w0 = w_next;
      nw = nw_next;
    }
    return write_slab(prev_slot, prev_bytes);
  };
  rc = run();
  if (rc) {
    slab_drain(f, d.stream);
    return rc;
  }
  if (count_out) *count_out = rank - ((flags & DSE_FINISH_HACK) ? 4 : 0);
  return DSE_OK;
}

uint32_t finish_flags_for(int32_t my_num) {
  return my_num == 1 ? (DSE_FINISH_DOUBLES | DSE_FINISH_HACK) : 0u;
}

int32_t finish_close(FILE* fp, const char* path, int32_t rc) {
  if (std::fclose(fp) != 0 && !rc) return fail(DSE_EIO, std::string("write failed: ") + path);
  return rc;
}

}  // namespace

extern "C" uint64_t dse_finish_text_bound(uint64_t g_start, uint64_t nbits, uint64_t count, uint32_t flags) {
  // every entry: ", " and a value no longer than the range's largest (the
  // printed length is monotone in the value; the hack literals are shorter
  // still); a "\n" after every tenth entry wherever the first rank falls, and
  // the closing one
  const uint64_t vmax = 3 + 2 * (g_start + (nbits ? nbits - 1 : 0));
  const uint64_t per = dse::fin_value_len(vmax, flags & DSE_FINISH_DOUBLES) + 2;
  if (count > (~0ull - 16) / (per + 1)) return ~0ull;
  return count * per + (count + 9) / 10 + 1;
}

extern "C" int32_t dse_finish_text_dev_async(dse_ctx* ctx, uint32_t flags, uint64_t g_start, uint64_t nbits,
                                             const uint64_t* mask_dev, uint64_t first_rank, void* text_dev,
                                             uint64_t text_cap, uint64_t* totals_dev, void* stream) {
  if (!ctx || !totals_dev) return fail(DSE_EINVAL, "null ctx or totals");
  if (nbits && !mask_dev) return fail(DSE_EINVAL, "null mask");
  if (text_cap && !text_dev) return fail(DSE_EINVAL, "null text buffer with a non-zero capacity");
  int32_t rc = finish_check_range(flags, g_start, nbits);
  if (rc) return rc;
  if (first_rank > (1ull << 62)) return fail(DSE_ERANGE, "first_rank beyond 2^62");
  DevState& d = ctx->devs[0];
  HIP_TRY(hipSetDevice(d.device));
  return finish_launch(d, flags, g_start, nbits, mask_dev, first_rank, text_dev, text_cap,
                       reinterpret_cast<unsigned long long*>(totals_dev), (hipStream_t)stream);
}

extern "C" int32_t dse_finish_resident_file(dse_ctx* ctx, const char* path, int32_t my_num) {
  if (!ctx || !path) return fail(DSE_EINVAL, "null ctx or path");
  if (my_num < 1) return fail(DSE_EINVAL, "my_num must be >= 1");
  DevState* d;
  uint64_t* mask;
  int32_t rc = find_resident(ctx, my_num, &d, &mask);
  if (rc) return rc;
  const uint64_t cs = (uint64_t)ctx->resident.cs;
  const uint32_t flags = finish_flags_for(my_num);
  const uint64_t g_start = (uint64_t)(my_num - 1) * cs;
  if ((rc = finish_check_range(flags, g_start, cs))) return rc;
  FILE* fp = std::fopen(path, "wb");
  if (!fp) return fail(DSE_EIO, std::string("cannot open ") + path);
  if (hipSetDevice(d->device) != hipSuccess) return finish_close(fp, path, fail(DSE_EHIP, "hipSetDevice failed"));
  rc = finish_pipeline(ctx, *d, fp, path, flags, g_start, cs, mask, nullptr);
  return finish_close(fp, path, rc);
}

extern "C" int32_t dse_finish_range_file(dse_ctx* ctx, const char* path, int32_t my_num, uint64_t g_start,
                                         uint64_t nbits, uint64_t* count) {
  if (!ctx || !path) return fail(DSE_EINVAL, "null ctx or path");
  if (my_num < 1) return fail(DSE_EINVAL, "my_num must be >= 1");
  const uint32_t flags = finish_flags_for(my_num);
  int32_t rc = finish_check_range(flags, g_start, nbits);
  if (rc) return rc;
  FILE* fp = std::fopen(path, "wb");
  if (!fp) return fail(DSE_EIO, std::string("cannot open ") + path);
  DevState& d = ctx->devs[0];
  uint64_t c = 0;
  if (nbits) {
    rc = sieve_range_host(ctx, d, g_start, nbits, nullptr, &c, true);
    if (!rc) rc = finish_pipeline(ctx, d, fp, path, flags, g_start, nbits, d.scratch_mask.as<uint64_t>(), nullptr);
  }
  rc = finish_close(fp, path, rc);
  if (!rc && count) *count = c;
  return rc;
}
