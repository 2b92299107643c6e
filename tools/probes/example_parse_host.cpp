// Host run of the device tf.train.Example parser (assembled_cnn_amd/csrc/example_parse.h) under the address and
// undefined-behaviour sanitizers.  The header's functions are the text example_parse_kernel and example_label_rows_kernel
// compile; here the lanes of the workgroup are a loop and every barrier is the end of that loop.
//
//   c++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread example_parse_host.cpp -o example_parse_host
//   example_parse_host cases.bin rows.bin [threads]
//
// cases.bin (tests/test_example_parse_host_sanitizer.py writes it; little endian): int32 count, int32 num_classes, then per
// case int64 n and the n payload bytes.  Every payload is copied into a heap block of its own that ends with the payload's
// last byte -- a byte read behind the span is an AddressSanitizer report -- and runs with its span starting at each offset
// 0..15 of a 16-byte vector, bytes of FF in front of it; the sixteen rows must agree.  rows.bin gets, per case, the
// asm_example_row of alignment 0 (so offsets are relative to the payload), the int32 status of the label routine and the 2 *
// num_classes words of its row, which start as A5A5A5A5.  The program prints the number of cases it ran.
#include "jpeg_probe.h"

#include "../../assembled_cnn_amd/csrc/example_parse.h"

#include <memory>

static const uint32_t kCanary = 0xA5A5A5A5u;

// what example_parse_kernel does for one span
static void parse_span(const uint8_t* buf, int64_t buf_bytes, const asm_span_desc& d, asm_example_row* row) {
  std::unique_ptr<exp_state> state(new exp_state);
  exp_state* s = state.get();
  exp_init(s, d.offset, d.length, buf_bytes);
  if (s->cls == 0) {
    const uint8_t* span = buf + d.offset;
    int r;
    do {
      for (int lane = 0; lane < EXP_LANES; ++lane) exp_load_window(s, span, d.length, lane);
      r = s->ret = exp_walk(s, d.length);
    } while (r == EXP_REFILL);
  }
  exp_row(s, d.offset, row);
}

// what example_label_rows_kernel does for one row
static int32_t label_row(const uint8_t* buf, int64_t buf_bytes, const asm_example_row& r, int num_classes, uint32_t* out) {
  const int32_t st = exl_status(r, num_classes, buf_bytes);
  if (st) return st;
  for (int col = 0; col < 2 * num_classes; ++col) out[col] = exl_word(buf, r, num_classes, col);
  return 0;
}

static bool same_row(const asm_example_row& a, const asm_example_row& b, int64_t shift) {
  if (a.cls != b.cls) return false;
  if (a.cls != 0) return true;
  return a.label == b.label && a.enc_offset == b.enc_offset + shift && a.name_offset == b.name_offset + shift &&
         a.logit_offset == b.logit_offset + shift && a.enc_length == b.enc_length && a.name_length == b.name_length &&
         a.logit_count == b.logit_count && a.n_boxes == b.n_boxes;
}

int main(int argc, char** argv) {
  int32_t count = 0, num_classes = 0;
  FILE* f = probe::open_cases(argc, argv, &count);
  if (!f || argc < 3 || !probe::read_exact(f, &num_classes, 4) || num_classes < 1 || num_classes > 4096) return 2;
  std::vector<std::vector<uint8_t>> cases((size_t)count);
  for (auto& c : cases)
    if (!probe::read_rows<int64_t>(f, &c, 1ll << 28)) return 2;
  fclose(f);
  const size_t words = 2 * (size_t)num_classes;
  std::vector<asm_example_row> rows(cases.size());
  std::vector<int32_t> status(cases.size());
  std::vector<uint32_t> labels(cases.size() * words, kCanary);
  std::atomic<long> ran{0}, accepted{0}, mismatches{0};
  char* shifted_argv[3] = {argv[0], argv[1], argc > 3 ? argv[3] : nullptr};
  probe::run_pool(cases.size(), argc > 3 ? 3 : 2, shifted_argv, [&](size_t k) {
    const int64_t n = (int64_t)cases[k].size();
    for (int align = 0; align < 16; ++align) {
      const int64_t front = 16, total = align + n;
      // exact size: a 16-byte aligned block of front + total bytes that ends with the span's last byte
      uint8_t* exact = (uint8_t*)::operator new((size_t)(front + total), std::align_val_t(16));
      memset(exact, 0xFF, (size_t)(front + align));
      if (n) memcpy(exact + front + align, cases[k].data(), (size_t)n);
      const asm_span_desc d = {(int64_t)front + align, n, 0u, 0u};
      asm_example_row r;
      parse_span(exact, (int64_t)front + total, d, &r);
      if (align == 0) {
        asm_example_row rel = r;
        if (r.cls == 0) {
          rel.enc_offset -= d.offset;
          rel.name_offset -= d.offset;
          rel.logit_offset -= d.offset;
        }
        rows[k] = rel;
        status[k] = label_row(exact, (int64_t)front + total, r, num_classes, &labels[k * words]);
      } else {
        asm_example_row shifted = rows[k];
        if (!same_row(r, shifted, d.offset) && mismatches++ < 20)
          fprintf(stderr, "case %zu: the row at alignment %d differs from the row at alignment 0\n", k, align);
        std::vector<uint32_t> again(words, kCanary);
        const int32_t st = label_row(exact, (int64_t)front + total, r, num_classes, again.data());
        if ((st != status[k] || memcmp(again.data(), &labels[k * words], 4 * words)) && mismatches++ < 20)
          fprintf(stderr, "case %zu: the label row at alignment %d differs from the one at alignment 0\n", k, align);
      }
      ::operator delete(exact, std::align_val_t(16));
    }
    ++ran;
    if (rows[k].cls == 0) ++accepted;
  });
  FILE* o = fopen(argv[2], "wb");
  if (!o) {
    perror(argv[2]);
    return 2;
  }
  for (size_t k = 0; k < cases.size(); ++k)
    if (fwrite(&rows[k], sizeof rows[k], 1, o) != 1 || fwrite(&status[k], 4, 1, o) != 1 ||
        fwrite(&labels[k * words], 4, words, o) != words)
      return 2;
  if (fclose(o)) return 2;
  printf("example_parse_host: %ld cases at 16 alignments, %ld class 0, %ld mismatches\n", ran.load(), accepted.load(),
         mismatches.load());
  return mismatches.load() ? 1 : 0;
}
