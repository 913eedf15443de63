// Memory-safety check of the JPEG host front end (csrc/jpeg_host.hip: mpn_jpeg_info, mpn_jpeg_entropy_decode,
// mpn_jpeg_scan_prepare, mpn_jpeg_scans_info, mpn_jpeg_scans_decode), meant to be built with -fsanitize=address,undefined and
// run on the CPU: tools/jpeg_host_fuzz.sh does both. It links nothing but that one source, compiled as plain C++.
//
//   jpeg_host_fuzz FILE...      the first three FILEs are also fed as every one of their prefixes
//
// Inputs: every file as it is (it must decode, unless its name holds "damaged_": then it may be refused); every prefix of
// the first three; kCorruptions single-byte corruptions of files drawn with the seeded generator below. The input bytes, the
// coefficient buffers and every struct an entry point fills are heap blocks of exactly their size, so a read or a write one
// byte outside any of them is an AddressSanitizer report. Exit status 0 = every call returned MPN_OK or a documented error.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../include/mpn.h"

void mpn_set_error(const char*, ...) {}         // the library's error text is not under test

namespace {

constexpr uint64_t kSeed = 0x5EED2026ull;
constexpr int kCorruptions = 2000;
constexpr int kPrefixFiles = 3;

struct Tally {
    long ok = 0, refused = 0, library = 0;
};

uint64_t next(uint64_t& s) {                    // xorshift64
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

template <class T>
T* block() { return (T*)malloc(sizeof(T)); }       // an exact-size block: writing past the struct is a report

// One input through the five entry points. Returns false on a return code the header does not document, or when the
// one-scan and the multi-scan view of a file both decode and disagree about its size.
bool feed(const uint8_t* bytes, size_t n, Tally& t, bool must_decode) {
    uint8_t* data = (uint8_t*)malloc(n ? n : 1);        // an exact-size block: reading past n is a report
    memcpy(data, bytes, n);
    mpn_jpeg_header* one = block<mpn_jpeg_header>();
    mpn_jpeg_scan_desc* prepared = block<mpn_jpeg_scan_desc>();
    mpn_jpeg_scans_header* h = block<mpn_jpeg_scans_header>();
    mpn_jpeg_desc* desc = block<mpn_jpeg_desc>();
    int rc = mpn_jpeg_info(data, n, one);
    bool fine = rc == MPN_OK || rc == MPN_ERR_BAD_DATA;
    if (rc == MPN_OK && one->supported) {
        int16_t* coefs = (int16_t*)malloc((size_t)one->coef_bytes);
        rc = mpn_jpeg_entropy_decode(data, n, coefs, (size_t)one->coef_bytes, desc);
        fine = fine && (rc == MPN_ERR_BAD_DATA || (rc == MPN_OK && desc->width == one->width && desc->total_blocks == one->total_blocks));
        free(coefs);
    }
    rc = mpn_jpeg_scan_prepare(data, n, prepared);
    fine = fine && (rc == MPN_ERR_BAD_DATA || (rc == MPN_OK && (!prepared->supported || (size_t)prepared->scan_offset <= n)));
    rc = mpn_jpeg_scans_info(data, n, h);
    fine = fine && (rc == MPN_OK || rc == MPN_ERR_BAD_DATA);
    if (rc == MPN_OK && h->route != MPN_JPEG_ROUTE_LIBRARY) {
        int16_t* coefs = (int16_t*)malloc((size_t)h->coef_bytes);
        rc = mpn_jpeg_scans_decode(data, n, coefs, (size_t)h->coef_bytes, desc);
        if (rc == MPN_OK) {
            ++t.ok;
            fine = fine && desc->width == h->width && desc->height == h->height && desc->total_blocks == h->total_blocks;
        } else {
            ++t.refused;
            fine = fine && rc == MPN_ERR_BAD_DATA;
        }
        free(coefs);
    } else if (rc == MPN_OK) {
        ++t.library;
    } else {
        ++t.refused;
    }
    free(desc);
    free(h);
    free(prepared);
    free(one);
    free(data);
    return fine && (!must_decode || rc == MPN_OK);
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<std::vector<uint8_t>> files;
    for (int i = 1; i < argc; ++i) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[i]);
            return 2;
        }
        std::vector<uint8_t> b;
        uint8_t chunk[4096];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) b.insert(b.end(), chunk, chunk + got);
        fclose(f);
        files.push_back(b);
    }
    if ((int)files.size() < kPrefixFiles) {
        fprintf(stderr, "usage: jpeg_host_fuzz FILE FILE FILE [FILE...]\n");
        return 2;
    }
    Tally whole, prefixes, corrupted;
    for (size_t i = 0; i < files.size(); ++i) {
        if (!feed(files[i].data(), files[i].size(), whole, strstr(argv[i + 1], "damaged_") == nullptr)) {
            fprintf(stderr, "%s does not decode, or an undocumented return code\n", argv[i + 1]);
            return 1;
        }
    }
    for (int i = 0; i < kPrefixFiles; ++i) {
        for (size_t n = 0; n < files[i].size(); ++n) {
            if (!feed(files[i].data(), n, prefixes, false)) {
                fprintf(stderr, "%s cut to %zu bytes: undocumented return code\n", argv[i + 1], n);
                return 1;
            }
        }
    }
    uint64_t s = kSeed;
    for (int k = 0; k < kCorruptions; ++k) {
        std::vector<uint8_t> b = files[next(s) % files.size()];
        const size_t at = next(s) % b.size();
        b[at] = (uint8_t)(b[at] ^ (1 + next(s) % 255));          // always another value
        if (!feed(b.data(), b.size(), corrupted, false)) {
            fprintf(stderr, "corruption %d: undocumented return code\n", k);
            return 1;
        }
    }
    printf("files       %ld decoded, %ld refused (the damaged ones)\n", whole.ok, whole.refused);
    printf("prefixes    %ld decoded, %ld refused, %ld left to a library\n", prefixes.ok, prefixes.refused, prefixes.library);
    printf("corruptions %ld decoded, %ld refused, %ld left to a library (seed 0x%llx)\n", corrupted.ok, corrupted.refused,
           corrupted.library, (unsigned long long)kSeed);
    return 0;
}
