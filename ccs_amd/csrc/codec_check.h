// codec_check.h — the argument check of the two BGZF codecs (include/ccsx.h "BGZF inflate on the device", "BGZF deflate on the device"), written once over a
// description of the codec's list item.  No HIP: codec_host.h builds the device path on it, the *_host entry points call it, and a plain C++ program can include it
// (tools/deflate_sanitize runs hostile lists through it under the sanitizers).  It needs ccsx.h and ccsx_set_error, nothing else.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "ccsx.h"

void ccsx_set_error(const std::string &s);

// What the check knows of a list item: its noun in the messages, the bytes of its output range, and the length that carries the 0 .. 65536 limit with its text.
struct ccsx_inflate_items {
    using Item = ccsx_deflate_block;
    static constexpr const char *noun = "block", *limit_text = "out_len outside 0 .. 65536";
    static constexpr int32_t limit = CCSX_INFLATE_MAX_OUT;
    static int32_t range(const Item &b) { return b.out_len; }
    static int32_t limited(const Item &b) { return b.out_len; }
};

struct ccsx_deflate_items {
    using Item = ccsx_deflate_span;
    static constexpr const char *noun = "span", *limit_text = "in_len outside 0 .. 65536";
    static constexpr int32_t limit = CCSX_DEFLATE_MAX_IN;
    static int32_t range(const Item &b) { return b.out_cap; }
    static int32_t limited(const Item &b) { return b.in_len; }
};

// The argument errors of a call, set under the exported function's name `fn`: nothing was enqueued or written when this fails.  `results`: the caller's result
// arrays are all there.  `order` is scratch.  Every sum and difference below is of values already known to lie in 0 .. the buffer's length: offsets at the ends of
// int64 are refused without overflow.
template <typename D> static int ccsx_codec_check(const char *fn, const uint8_t *src, int64_t src_len, const typename D::Item *items, int32_t n, const uint8_t *dst,
                                                  int64_t dst_len, bool results, std::vector<int32_t> &order)
{
    using Item = typename D::Item;
    const std::string f(fn), noun(D::noun);
    if (src_len < 0 || dst_len < 0 || n < 0) { ccsx_set_error(f + ": negative size"); return -1; }
    if ((n > 0 && (!items || !results)) || (src_len > 0 && !src) || (dst_len > 0 && !dst)) { ccsx_set_error(f + ": null argument"); return -1; }
    const auto refuse = [&](int32_t i, const char *what) { ccsx_set_error(f + ": " + noun + " " + std::to_string(i) + ": " + what); return -1; };
    bool monotone = true;
    for (int32_t i = 0; i < n; ++i) {
        const Item &b = items[i];
        if (D::limited(b) < 0 || D::limited(b) > D::limit) return refuse(i, D::limit_text);
        if (b.in_len < 0 || b.in_off < 0 || b.in_off > src_len - b.in_len) return refuse(i, "input range outside src");
        if (D::range(b) < 0 || b.out_off < 0 || b.out_off > dst_len - D::range(b)) return refuse(i, "output range outside dst");
        if (i && b.out_off < items[i - 1].out_off + D::range(items[i - 1])) monotone = false;
    }
    if (!monotone) {                 // (a BGZF reader's or writer's items are in order: the sort is for everyone else).  Empty ranges overlap nothing and are left out
        order.clear();
        for (int32_t i = 0; i < n; ++i) if (D::range(items[i]) > 0) order.push_back(i);
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return items[a].out_off < items[b].out_off; });
        for (size_t k = 1; k < order.size(); ++k) {
            const Item &p = items[order[k - 1]], &q = items[order[k]];
            if (q.out_off < p.out_off + D::range(p)) {
                ccsx_set_error(f + ": " + noun + "s " + std::to_string(order[k - 1]) + " and " + std::to_string(order[k]) + ": output ranges overlap"); return -1;
            }
        }
    }
    return 0;
}
