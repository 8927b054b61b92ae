// The packed operand images of the weights: the bf16 (or fp32) copies the GEMMs and chain kernels read, and the images derived
// from them (transposes, streamed MFMA fragments).  ONE table per handle (recnet_handle::wimg, filled by build_weight_images in
// api.hip once the chain eligibility is known) says which parameter tensor goes where, through which window, in what size; the
// workspace carve, the optimiser's pack descriptors (PackDesc), recnet_pack_weights, the refreshes of the derived images and
// the stale check (recnet_debug_images_stale) all read it.  A new image, or a changed leading dimension, is one row here.
#pragma once
struct recnet_handle;

// rows of the table, in the order the workspace holds them
enum WImageId {
  WI_U_W, WI_WC_W, WI_WE_W, WI_WCOMB, WI_WCOMBT, WI_WO_W,                       // decoder
  WI_WOR_W,                                                                     // both reconstructors
  WI_WOT, WI_WHHT, WI_WIH_F, WI_WHH_W,                                          // global reconstructor
  WI_WR4_W, WI_UR_W, WI_WR_W, WI_WIHH_W, WI_WST, WI_WIHHT, WI_WSTT,             // local reconstructor
  WI_COUNT
};
// how a derived image follows its source
enum WImageHow { WI_DIRECT, WI_TRANSPOSE, WI_STREAM_FWD /* lc_pack_stream_kernel */, WI_STREAM_BWD /* lcbig_pack_stream_kernel */ };

// One window of a parameter tensor [.][tcols] (index t in dec_list / rec_list order) inside a direct image: source element
// (r, c) with r in [r0, r0 + nr) and c in [c0, c0 + nc) goes to image element (dr + r - r0, dc + c - c0).  Recurrent weights
// land in the 4-block gate layout through row windows (W_ih of a GRU: 3 blocks in place, the 4th stays zero; W_hh of a GRU:
// blocks (r, z) in place, block n -> packed block 3, packed block 2 stays zero; see gru_point).
struct WImageSrc { int t, tcols, c0, nc, r0, nr; size_t dr; int dc; };
#define WI_MAX_SRC 6

struct WImage {
  void* recnet_handle::* field = nullptr;   // the handle field that receives the pointer (null: not an image of this handle's kind)
  int group = 0;                            // optimiser group whose parameters it follows: 0 decoder, 1 reconstructor
  size_t rows = 0; int cols = 0, ld = 0;    // logical extent and leading dimension, elements (a fragment image: [fragments][8])
  bool frag = false;                        // streamed-fragment image: bf16 whatever the precision, carved with its own slack
  bool carved = false;                      // has room in the workspace
  bool live = false;                        // kept current (packed / refreshed) and compared by the stale check
  int how = WI_DIRECT, from = -1;           // derived images: their source image and what produces them
  int nsrc = 0; WImageSrc src[WI_MAX_SRC];  // direct images: their windows
};

// 16-byte fragments of a streamed image: [owner workgroups][4 waves][streamed k-steps][4][64 lanes] (loc_chain.hpp, loc_big.hpp)
static inline size_t wimg_stream_fragments(int owners, int streamed_steps) { return (size_t)owners * 4 * streamed_steps * 4 * 64; }
// what the carve takes for an image, in floats: operand images are sized as if fp32 (the bf16 path uses half of each)
static inline size_t wimg_take_floats(const WImage& im) { return im.frag ? im.rows * im.ld / 2 + 64 : im.rows * (size_t)im.ld; }
static inline size_t wimg_bytes(const WImage& im, int lp) { return im.rows * (size_t)im.ld * (lp ? 2 : 4); }
