// Stand-alone robustness check of csrc/jpeg_entropy.h, meant to be built for the host with -fsanitize=address,undefined:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I bioscan-clip_amd/csrc \
//       tools/jpeg_entropy_check.cpp -o /tmp/jpeg_entropy_check && /tmp/jpeg_entropy_check tests/golden/jpeg
//
// Every *.jpg of the directory is decoded intact (files whose name starts with 'p' are the refusal fixtures and must be refused),
// then truncated at every length, then with each of its first 600 bytes replaced by 0x00, 0xFF and its complement, one byte at a
// time.  Each call must return 0 or one of the documented error codes, and must leave the guard bands around the coefficient,
// table and record buffers untouched.  The input is copied into a heap block of exactly its length for every call, so the
// sanitiser sees any read past its end.  Exit status 0 = all held.
#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "jpeg_entropy.h"

namespace {

constexpr size_t GUARD = 256;   // int16 elements on either side of the coefficient buffer
constexpr uint16_t FILL = 0xA5C3;

struct Arena {
    std::vector<uint16_t> coef;   // guard | capacity | guard
    std::vector<uint16_t> qtab;   // guard | 192 | guard
    std::vector<int32_t> rec;     // guard | 16 | guard
    size_t capacity = 0;
    void reset(size_t cap) {
        capacity = cap;
        coef.assign(cap + 2 * GUARD, FILL);
        qtab.assign(192 + 2 * GUARD, FILL);
        rec.assign(bsclip_jpeg::REC + 2 * GUARD, (int32_t)0xA5C3A5C3);
    }
    bool guards_ok() const {
        for (size_t i = 0; i < GUARD; ++i) {
            if (coef[i] != FILL || coef[GUARD + capacity + i] != FILL) return false;
            if (qtab[i] != FILL || qtab[GUARD + 192 + i] != FILL) return false;
            if (rec[i] != (int32_t)0xA5C3A5C3 || rec[GUARD + bsclip_jpeg::REC + i] != (int32_t)0xA5C3A5C3) return false;
        }
        return true;
    }
};

bool known_code(int rc) { return rc == 0 || rc == -1 || (rc <= -10 && rc >= -18); }

long g_calls = 0, g_ok = 0, g_failures = 0;

int run(const std::vector<uint8_t>& data, Arena& a, const char* what, size_t at) {
    uint8_t* copy = static_cast<uint8_t*>(malloc(data.size() ? data.size() : 1));   // exact length: over-reads are the sanitiser's
    std::copy(data.begin(), data.end(), copy);
    char msg[160] = "";
    const int rc = bsclip_jpeg::entropy_decode(copy, data.size(), reinterpret_cast<int16_t*>(a.coef.data() + GUARD), (int64_t)a.capacity,
                                               a.qtab.data() + GUARD, a.rec.data() + GUARD, msg, sizeof(msg));
    free(copy);
    ++g_calls;
    g_ok += rc == 0;
    if (!known_code(rc) || (rc != 0 && !msg[0]) || !a.guards_ok()) {
        fprintf(stderr, "FAIL %s at %zu: rc=%d msg='%s' guards %s\n", what, at, rc, msg, a.guards_ok() ? "intact" : "OVERWRITTEN");
        ++g_failures;
        a.reset(a.capacity);
    }
    return rc;
}

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
            if (n.size() > 4 && n.substr(n.size() - 4) == ".jpg") names.push_back(n);
        }
        closedir(d);
    }
    std::sort(names.begin(), names.end());
    if (names.empty()) {
        fprintf(stderr, "no .jpg files in %s\n", argv[1]);
        return 2;
    }
    Arena a;
    for (const std::string& name : names) {
        const std::vector<uint8_t> data = slurp(std::string(argv[1]) + "/" + name);
        bsclip_jpeg::Decoder probe;
        const int prc = probe.parse(data.data(), data.size());
        const bool refusal = name[0] == 'p';
        if ((prc == 0) == refusal) {
            fprintf(stderr, "FAIL %s: probe returned %d (%s)\n", name.c_str(), prc, probe.msg);
            ++g_failures;
            continue;
        }
        const size_t count = prc == 0 ? (size_t)probe.f.coef_count : 64;
        // exact capacity, then a roomy one under which a stream whose damaged header declares a larger image is decoded, not turned away
        for (const size_t cap : {count, count * 16}) {
            a.reset(cap);
            const int rc = run(data, a, name.c_str(), data.size());
            if ((rc == 0) == refusal || rc != prc) {
                fprintf(stderr, "FAIL %s intact: rc=%d, probe said %d\n", name.c_str(), rc, prc);
                ++g_failures;
            }
            for (size_t len = 0; len < data.size(); ++len) run(std::vector<uint8_t>(data.begin(), data.begin() + (long)len), a, "truncation", len);
            std::vector<uint8_t> m = data;
            for (size_t i = 0; i < std::min<size_t>(600, data.size()); ++i) {
                for (const uint8_t v : {(uint8_t)0x00, (uint8_t)0xFF, (uint8_t)~data[i]}) {
                    if (v == data[i]) continue;
                    m[i] = v;
                    run(m, a, "corruption", i);
                }
                m[i] = data[i];
            }
        }
    }
    printf("jpeg_entropy_check: %zu files, %ld calls, %ld decoded, %ld failures\n", names.size(), g_calls, g_ok, g_failures);
    return g_failures ? 1 : 0;
}
