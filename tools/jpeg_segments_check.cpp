// Stand-alone check of the segment decoder that host and device share (csrc/jpeg_segment.h) and of the sync index
// (csrc/jpeg_entropy.h), meant to be built for the host with -fsanitize=address,undefined:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I bioscan-clip_amd/csrc \
//       tools/jpeg_segments_check.cpp -o /tmp/jpeg_segments_check && /tmp/jpeg_segments_check tests/golden/jpeg
//
// For every decodable *.jpg of the directory and sync_mcus in {1, 2, 3, 5}: the index is built, its segments are decoded in REVERSE
// order, each from its entry alone, into a buffer pre-filled with a guard pattern; the result must equal the sequential decode, every
// status must be 0 and the guard past the end must be intact.  Then the index stays as it is and the stream is damaged -- each of
// its first 600 scan bytes set to 0x00, 0xFF and its complement, and the stream cut at every length -- and every segment is decoded
// again: the routine must return (the sanitisers see any read outside the exact-length copy of the bytes and any write outside
// the buffer) and leave the guard alone.  A damaged byte can still be a valid code, so the number of damaged streams that gave
// status 0 with different coefficients is printed, not gated.  "flagged" lines name the first detected damage of each kind per
// file at sync_mcus = 2; tests/test_67_jpeg_entropy_gpu.py replays three of them on the device.  Exit status 0 = all held.
#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "jpeg_entropy.h"
#include "jpeg_segment.h"

namespace {

using namespace bsclip_jpeg;
constexpr size_t GUARD = 256;   // int16 elements past the end of the coefficient buffer
constexpr uint16_t FILL = 0xA5C3;

long g_decodes = 0, g_failures = 0, g_undetected = 0, g_detected = 0;

std::vector<uint8_t> slurp(const std::string& path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return v;
    uint8_t buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

struct Image {
    SegGeom g;
    int restart;
    SegHuff tabs[SEG_TABLES];
    size_t count;                   // coefficients
    std::vector<int16_t> want;      // the sequential decode
};

// every segment of `index`, last first, from an exact-length heap copy of `data`; returns the or of the statuses
int decode_all(const Image& im, const std::vector<uint8_t>& data, const std::vector<int32_t>& index, int sync_mcus, int16_t* coef) {
    uint8_t* copy = static_cast<uint8_t*>(malloc(data.size() ? data.size() : 1));
    std::copy(data.begin(), data.end(), copy);
    const int nseg = (int)(index.size() / SYNC_ENTRY);
    int all = 0;
    for (int j = nseg - 1; j >= 0; --j) {
        int first, cnt;
        bool chained;
        segment_range(j, im.g.nmcu, im.restart, sync_mcus, &first, &cnt, &chained);
        all |= decode_segment_checked<true>(copy, (uint32_t)data.size(), index.data() + (size_t)j * SYNC_ENTRY, first, cnt, im.g, im.tabs, coef,
                                            index.data() + (size_t)(chained ? j + 1 : j) * SYNC_ENTRY, chained);
        ++g_decodes;
    }
    free(copy);
    return all;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <directory of .jpg fixtures>\n", argv[0]);
        return 2;
    }
    std::vector<std::string> names;
    if (DIR* d = opendir(argv[1])) {
        while (dirent* e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() > 4 && n.substr(n.size() - 4) == ".jpg" && n[0] != 'p') names.push_back(n);   // 'p...' are the refusal fixtures
        }
        closedir(d);
    }
    std::sort(names.begin(), names.end());
    if (names.empty()) {
        fprintf(stderr, "no .jpg files in %s\n", argv[1]);
        return 2;
    }
    for (const std::string& name : names) {
        const std::vector<uint8_t> data = slurp(std::string(argv[1]) + "/" + name);
        Decoder d;
        Image im;
        int sel = 0;
        if (d.parse(data.data(), data.size()) != OK || seg_tables(d, im.tabs, &sel) != OK) {
            fprintf(stderr, "FAIL %s: headers refused (%s)\n", name.c_str(), d.msg);
            ++g_failures;
            continue;
        }
        im.g = seg_geom(d.f, sel);
        im.restart = d.f.restart;
        im.count = (size_t)d.f.coef_count;
        im.want.assign(im.count, 0);
        const size_t scan = d.f.scan_pos;
        {
            uint16_t qtab[192];
            int32_t rec[REC];
            char msg[160] = "";
            if (entropy_decode(data.data(), data.size(), im.want.data(), (int64_t)im.count, qtab, rec, msg, sizeof(msg)) != OK) {
                fprintf(stderr, "FAIL %s: sequential decode refused (%s)\n", name.c_str(), msg);
                ++g_failures;
                continue;
            }
        }
        // 16-byte aligned, as the routine requires of a coefficient buffer
        int16_t* coef = static_cast<int16_t*>(aligned_alloc(16, (im.count + GUARD) * sizeof(int16_t) + 16 - ((im.count + GUARD) * sizeof(int16_t)) % 16));
        auto refill = [&] { std::fill(reinterpret_cast<uint16_t*>(coef), reinterpret_cast<uint16_t*>(coef) + im.count + GUARD, FILL); };
        auto guard_ok = [&] {
            for (size_t i = 0; i < GUARD; ++i)
                if (reinterpret_cast<uint16_t*>(coef)[im.count + i] != FILL) return false;
            return true;
        };
        for (const int s : {1, 2, 3, 5}) {
            char msg[160] = "";
            const int64_t n = sync_index(data.data(), data.size(), s, nullptr, 0, msg, sizeof(msg));
            if (n != segment_count(im.g.nmcu, im.restart, s)) {
                fprintf(stderr, "FAIL %s sync %d: %lld entries (%s)\n", name.c_str(), s, (long long)n, msg);
                ++g_failures;
                continue;
            }
            std::vector<int32_t> index((size_t)n * SYNC_ENTRY, -1);
            if (sync_index(data.data(), data.size(), s, index.data(), n, msg, sizeof(msg)) != n) {
                fprintf(stderr, "FAIL %s sync %d: index refused (%s)\n", name.c_str(), s, msg);
                ++g_failures;
                continue;
            }
            refill();
            const int st = decode_all(im, data, index, s, coef);
            if (st != 0 || !std::equal(im.want.begin(), im.want.end(), coef) || !guard_ok()) {
                fprintf(stderr, "FAIL %s sync %d intact: status %d, coefficients %s, guard %s\n", name.c_str(), s, st,
                        std::equal(im.want.begin(), im.want.end(), coef) ? "equal" : "DIFFER", guard_ok() ? "intact" : "OVERWRITTEN");
                ++g_failures;
            }
            auto damaged = [&](const std::vector<uint8_t>& m, const char* what, size_t at, unsigned value, bool* announced) {
                refill();
                const int dst = decode_all(im, m, index, s, coef);
                if (!guard_ok()) {
                    fprintf(stderr, "FAIL %s sync %d %s at %zu: guard OVERWRITTEN\n", name.c_str(), s, what, at);
                    ++g_failures;
                }
                if (dst != 0) {
                    ++g_detected;
                    if (announced && !*announced && s == 2) {
                        printf("flagged %s sync=2 scan+%zu value=0x%02X status=%d\n", name.substr(0, name.size() - 4).c_str(), at - scan, value, dst);
                        *announced = true;
                    }
                } else if (!std::equal(im.want.begin(), im.want.end(), coef)) {
                    ++g_undetected;
                }
            };
            std::vector<uint8_t> m = data;
            bool announced[3] = {false, false, false};
            for (size_t i = scan; i < std::min(scan + 600, data.size()); ++i) {
                const uint8_t vals[3] = {0x00, 0xFF, (uint8_t)~data[i]};
                for (int k = 0; k < 3; ++k) {
                    if (vals[k] == data[i]) continue;
                    m[i] = vals[k];
                    damaged(m, "corruption", i, vals[k], &announced[k]);
                }
                m[i] = data[i];
            }
            for (size_t len = 0; len < data.size(); ++len)
                damaged(std::vector<uint8_t>(data.begin(), data.begin() + (long)len), "truncation", len, 0, nullptr);
        }
        free(coef);
    }
    printf("jpeg_segments_check: %zu files, %ld segment decodes, %ld damaged streams flagged, %ld gave status 0 with different coefficients, "
           "%ld failures\n",
           names.size(), g_decodes, g_detected, g_undetected, g_failures);
    return g_failures ? 1 : 0;
}
