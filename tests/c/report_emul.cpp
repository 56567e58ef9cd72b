/*
 * report_emul — vsa_hs_report_records_emulated (the device path's passes,
 * buffer sizing and block table, run in serial loops on the CPU) against
 * vsa_hs_report_records_host, field for field, over synthetic sorted records:
 * small shapes, and 4 blocks of 256 MiB of offsets with ~200k records spread
 * over the 1 GiB range, with the uniform and a non-uniform block table.
 *
 * Built by `make report-emul-asan` with AddressSanitizer and UBSan on the
 * host code that holds the passes; needs no GPU.  Exit status 0 = every
 * comparison equal.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vectorscan_amd_hs.h"

namespace {

struct Rng {
    uint64_t s;
    uint64_t next() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    }
    uint64_t below(uint64_t n) { return next() % n; }
};

struct Set {
    const char *name;
    std::vector<std::string> exprs;
    std::vector<unsigned> flags, ids;
};

const unsigned H = VSA_HS_FLAG_SINGLEMATCH, L = VSA_HS_FLAG_SOM_LEFTMOST,
               I = VSA_HS_FLAG_CASELESS;
const char *LONG_A = "0123456789abcdefgh", *LONG_B = "QRSTUVWXyzyzyzyz";

std::vector<Set> sets() {
    return {
        {"short", {"abc", "bc", "xyz", "c"}, {0, 0, I, 0}, {1, 2, 3, 4}},
        {"long", {LONG_A, LONG_B, "efgh", "yzyz", "fgh"}, {0, I, 0, 0, 0}, {1, 2, 3, 4, 3}},
        {"keys", {"once", "ce", "bc", "abc", "yz", "xyz", LONG_A, "gh", "h"},
         {H, H, 0, 0, L, L, H, H, 0}, {1, 1, 3, 3, 8, 8, 6, 7, 3}},
    };
}

vsa_hs_database_t *compile(const Set &s) {
    std::vector<const char *> e;
    std::vector<size_t> lens;
    for (const auto &x : s.exprs) {
        e.push_back(x.c_str());
        lens.push_back(x.size());
    }
    vsa_hs_database_t *db = nullptr;
    vsa_hs_compile_error_t *err = nullptr;
    if (vsa_hs_compile_lit_multi(e.data(), s.flags.data(), s.ids.data(), lens.data(),
                                 (unsigned)e.size(), VSA_HS_MODE_BLOCK, nullptr, &db,
                                 &err) != VSA_HS_SUCCESS) {
        fprintf(stderr, "compile %s: %s\n", s.name, err ? err->message : "?");
        exit(2);
    }
    return db;
}

struct Records {
    std::vector<uint64_t> keys;
    std::vector<uint32_t> ids;
    void add(uint64_t end, uint32_t frag) {
        uint32_t order = 0;
        if (!keys.empty() && (keys.back() >> 24) == end) order = (uint32_t)(keys.back() & 0xffffff) + 1;
        keys.push_back(end << 24 | order);
        ids.push_back(frag);
    }
};

/* ~n ends rising over [0, size): at most ends a few random fragments, at
 * every `plant`-th one a long literal written so that it ends there and a
 * record of every fragment */
Records make_records(Rng &r, uint8_t *image, uint64_t size, uint64_t n, unsigned frags,
                     uint64_t plant) {
    Records rec;
    const uint64_t step = size / n ? size / n : 1;
    uint64_t k = 0;
    for (uint64_t at = 20 + r.below(step); at < size; at += 1 + r.below(2 * step), k++) {
        if (plant && k % plant == 0) {
            const char *w = (k / plant) % 2 ? LONG_B : LONG_A;
            memcpy(image + at + 1 - strlen(w), w, strlen(w));
            for (unsigned f = 0; f < frags; f++) rec.add(at, f);
            continue;
        }
        const unsigned m = 1 + (unsigned)r.below(3);
        for (unsigned j = 0; j < m; j++) rec.add(at, (uint32_t)r.below(frags));
    }
    return rec;
}

struct Result {
    int rc;
    uint64_t total;
    std::vector<uint64_t> counts, digests;
    std::vector<vsa_hs_match_t> m;
};

typedef int (*ReportFn)(const vsa_hs_database_t *, const uint64_t *, const uint32_t *, uint64_t,
                        const uint8_t *, const uint64_t *, const uint64_t *, uint32_t, uint64_t *,
                        uint64_t *, vsa_hs_match_t *, uint64_t, uint64_t *);

Result run(ReportFn fn, const vsa_hs_database_t *db, const Records &rec, const uint8_t *image,
           const std::vector<uint64_t> &offs, const std::vector<uint64_t> &lens) {
    Result o;
    const uint32_t nb = (uint32_t)offs.size();
    o.counts.assign(nb, 0);
    o.digests.assign(nb, 0);
    o.total = 0;
    o.rc = fn(db, rec.keys.data(), rec.ids.data(), rec.keys.size(), image, offs.data(),
              lens.data(), nb, nullptr, nullptr, nullptr, 0, &o.total);
    if (o.rc != VSA_HS_SUCCESS) return o;
    o.m.resize(o.total);
    uint64_t again = 0;
    o.rc = fn(db, rec.keys.data(), rec.ids.data(), rec.keys.size(), image, offs.data(),
              lens.data(), nb, o.counts.data(), o.digests.data(), o.m.data(), o.total, &again);
    if (again != o.total) o.rc = -100;
    return o;
}

int failures = 0;

void compare(const char *what, const vsa_hs_database_t *db, const Records &rec,
             const uint8_t *image, const std::vector<uint64_t> &offs,
             const std::vector<uint64_t> &lens) {
    const Result h = run(vsa_hs_report_records_host, db, rec, image, offs, lens);
    const Result e = run(vsa_hs_report_records_emulated, db, rec, image, offs, lens);
    bool ok = h.rc == VSA_HS_SUCCESS && e.rc == VSA_HS_SUCCESS && h.total == e.total &&
              h.counts == e.counts && h.digests == e.digests && h.m.size() == e.m.size();
    for (size_t k = 0; ok && k < h.m.size(); k++)
        ok = h.m[k].id == e.m[k].id && h.m[k].block == e.m[k].block &&
             h.m[k].from == e.m[k].from && h.m[k].to == e.m[k].to;
    printf("%-40s %8zu records %8llu matches  %s\n", what, rec.keys.size(),
           (unsigned long long)h.total, ok ? "equal" : "DIFFERENT");
    if (!ok) {
        fprintf(stderr, "  host rc %d total %llu, emulated rc %d total %llu\n", h.rc,
                (unsigned long long)h.total, e.rc, (unsigned long long)e.total);
        failures++;
    }
}

} // namespace

int main() {
    Rng r{0x9E3779B97F4A7C15ULL};
    const uint64_t MiB = 1ULL << 20;
    for (const Set &s : sets()) {
        vsa_hs_database_t *db = compile(s);
        unsigned frags = 0;
        vsa_hs_database_hwlm(db, nullptr, nullptr, &frags);
        std::string what;
        /* small: 6000 bytes, ragged blocks with gaps, an empty one, out of
         * offset order; then no records, and no blocks */
        {
            std::vector<uint8_t> image(6000, '.');
            Records rec = make_records(r, image.data(), image.size(), 900, frags, 7);
            what = std::string(s.name) + " small ragged";
            compare(what.c_str(), db, rec, image.data(), {3000, 0, 1000, 2500, 3290, 10},
                    {290, 1000, 1500, 0, 2710, 0});
            what = std::string(s.name) + " small uniform";
            compare(what.c_str(), db, rec, image.data(), {0, 2000, 4000}, {2000, 2000, 1990});
            what = std::string(s.name) + " no records";
            compare(what.c_str(), db, Records(), image.data(), {0, 2000}, {2000, 2000});
            what = std::string(s.name) + " no blocks";
            compare(what.c_str(), db, rec, image.data(), {}, {});
        }
        /* 4 blocks of 256 MiB: ~200k records over 1 GiB */
        {
            const uint64_t size = 1024 * MiB;
            uint8_t *image = (uint8_t *)calloc(size, 1);
            if (!image) {
                fprintf(stderr, "calloc of 1 GiB failed\n");
                return 2;
            }
            Records rec = make_records(r, image, size, 200000, frags, 5000);
            what = std::string(s.name) + " 4 x 256 MiB uniform";
            compare(what.c_str(), db, rec, image,
                    {0, 256 * MiB, 512 * MiB, 768 * MiB},
                    {256 * MiB, 256 * MiB, 256 * MiB, 256 * MiB});
            what = std::string(s.name) + " 4 x 256 MiB non-uniform";
            compare(what.c_str(), db, rec, image,
                    {768 * MiB + 9, 0, 300 * MiB, 512 * MiB, 256 * MiB + 3},
                    {256 * MiB - 9, 256 * MiB, 0, 256 * MiB - 1, 256 * MiB - 3});
            free(image);
        }
        vsa_hs_free_database(db);
    }
    if (failures) printf("report_emul: %d comparisons differ\n", failures);
    else printf("report_emul: all equal\n");
    return failures ? 1 : 0;
}
