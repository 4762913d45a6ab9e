// stream_pack_main.cpp — stand-alone driver of the host packers (host_pack.cpp), built by `make sanitize-streams` with
// -fsanitize=address,undefined into pack_streams_san: all three weight streams (forward blob, backward stream,
// input-gradient slices in its three flag combinations) of the corner networks in the four training modes, every
// buffer exactly as large as the size queries say.  Exit status 0 = every call succeeded and no sanitizer report.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fsnerf_hip.h"

struct Net {
  const char* name;
  int n_layers, d_hidden;
  uint32_t skip_mask;
  int n_freqs_pos, n_freqs_dir;
};

// tests/wstream_ref.py CORNERS, and 6 x 128 with skips (1, 3)
static const Net kNets[] = {
    {"min", 2, 128, 0u, 10, 4},           {"bare", 2, 128, 1u, 0, 0},         {"deep", 16, 128, 0x7fffu, 10, 4},
    {"wide-skips", 8, 256, 0x7fu, 10, 4}, {"wide-min", 2, 256, 0u, 10, 4},    {"6x128", 6, 128, 0xau, 10, 4},
};

static int fail(const char* what, const Net& n, int prec) {
  std::fprintf(stderr, "%s failed for %s, mode %d: %s\n", what, n.name, prec, fsn_last_error());
  return 1;
}

int main() {
  const int precs[] = {FSN_PREC_BF16X3, FSN_PREC_BF16, FSN_PREC_FP16X3, FSN_PREC_FP16};
  const int flags[][2] = {{1, 0}, {0, 1}, {1, 1}};
  uint32_t rng = 12345u;
  long long total = 0;
  for (const Net& n : kNets) {
    fsn_mlp_desc d{};
    d.n_layers = n.n_layers; d.d_hidden = n.d_hidden; d.skip_mask = n.skip_mask;
    d.n_freqs_pos = n.n_freqs_pos; d.n_freqs_dir = n.n_freqs_dir;
    for (int i = 0; i < 16; ++i) d.freqs_pos[i] = d.freqs_dir[i] = (float)(1 << (i & 7));
    const int L = n.n_layers, D = n.d_hidden, d_pe = 3 * (1 + 2 * n.n_freqs_pos), d_de = 3 * (1 + 2 * n.n_freqs_dir);
    // state_dict shapes: layers.0 .., sigma, connection, branch, rgb - each buffer exactly its tensor
    std::vector<std::vector<float>> W(L + 4), B(L + 4);
    for (int l = 0; l < L; ++l) {
      const bool wide = l > 0 && ((n.skip_mask >> (l - 1)) & 1u);
      W[l].resize((size_t)D * (l == 0 ? d_pe : D + (wide ? d_pe : 0)));
      B[l].resize(D);
    }
    W[L].resize(D); B[L].resize(1);
    W[L + 1].resize((size_t)D * D); B[L + 1].resize(D);
    W[L + 2].resize((size_t)(D / 2) * (D + d_de)); B[L + 2].resize(D / 2);
    W[L + 3].resize((size_t)3 * (D / 2)); B[L + 3].resize(3);
    std::vector<const float*> Wp(L + 4), Bp(L + 4);
    for (int i = 0; i < L + 4; ++i) {
      for (float& v : W[i]) { rng = rng * 1664525u + 1013904223u; v = ((int)(rng >> 8) - (1 << 23)) * (1.0f / (1 << 25)); }
      for (float& v : B[i]) { rng = rng * 1664525u + 1013904223u; v = ((int)(rng >> 8) - (1 << 23)) * (1.0f / (1 << 25)); }
      Wp[i] = W[i].data(); Bp[i] = B[i].data();
    }
    for (int prec : precs) {
      const int64_t fb = fsn_mlp_blob_bytes(&d, prec);
      if (fb <= 0) return fail("fsn_mlp_blob_bytes", n, prec);
      std::vector<unsigned char> blob((size_t)fb);
      if (fsn_mlp_pack_host(&d, prec, Wp.data(), Bp.data(), blob.data()) != FSN_OK) return fail("fsn_mlp_pack_host", n, prec);
      total += fb;
      for (int k = 0; k < 4; ++k) {  // the backward stream, then the slices' three flag combinations
        const int kind = k == 0 ? FSN_WSTREAM_BWD : FSN_WSTREAM_INPUT_GRAD;
        const int wx = k == 0 ? 0 : flags[k - 1][0], wd = k == 0 ? 0 : flags[k - 1][1];
        const int64_t sb = fsn_weight_stream_bytes(&d, prec, kind, wx, wd);
        if (sb <= 0) return fail("fsn_weight_stream_bytes", n, prec);
        std::vector<unsigned char> st((size_t)sb);
        if (fsn_weight_stream_pack_host(&d, prec, kind, wx, wd, Wp.data(), st.data()) != FSN_OK)
          return fail("fsn_weight_stream_pack_host", n, prec);
        total += sb;
      }
    }
  }
  std::printf("packed %lld bytes\n", total);
  return 0;
}
