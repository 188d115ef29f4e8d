// Stand-alone fuzz driver of the host JPEG decoder (csrc/jpeg_host.h), built by tests/test_cpu_jpeg.py with g++ -fsanitize=address,undefined and run as a
// child process; never loaded into Python.  argv[1]: the file whose every truncation length is decoded; argv[2]: the file that gets 200 seeded
// single-byte corruptions.  Every call must return success or an error WITH a message; the coefficient and table buffers are heap blocks of exactly the
// size handed in (the sanitizer sees the first byte past them) and carry guard words of their own as well.  Exit status 0 = all held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../object-detection-tensorflow_amd/csrc/jpeg_host.h"

static std::vector<unsigned char> read_file(const char* path) {
    std::vector<unsigned char> v;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    unsigned char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static int failures = 0, accepted = 0, refused = 0;

// one decode of `n` bytes copied into a heap block of exactly n bytes; capacity: coefficient elements offered (-1 = what the picture needs)
static void run(const unsigned char* data, size_t n, long long capacity, const char* what, long long arg) {
    unsigned char* d = (unsigned char*)malloc(n ? n : 1);
    memcpy(d, data, n);
    char err[512] = "";
    struct odtk_jpeg_info info;
    int rc = odtk_jpeg::info(d, n, &info, err, sizeof(err));
    if (rc != 0 && err[0] == 0) { fprintf(stderr, "%s %lld: info failed without a message\n", what, arg); ++failures; }
    if (rc == 0) {
        const size_t cap = capacity >= 0 ? (size_t)capacity : (size_t)info.coef_count;
        const size_t G = 8;
        int16_t* coef = (int16_t*)malloc((cap + 2 * G) * sizeof(int16_t));
        uint16_t* qt = (uint16_t*)malloc((256 + 2 * G) * sizeof(uint16_t));
        for (size_t i = 0; i < cap + 2 * G; ++i) coef[i] = (int16_t)0x5a5a;
        for (size_t i = 0; i < 256 + 2 * G; ++i) qt[i] = 0xa5a5;
        err[0] = 0;
        rc = odtk_jpeg::entropy_decode(d, n, coef + G, cap, qt + G, err, sizeof(err));
        if (rc != 0 && err[0] == 0) { fprintf(stderr, "%s %lld: decode failed without a message\n", what, arg); ++failures; }
        for (size_t i = 0; i < G; ++i)
            if (coef[i] != (int16_t)0x5a5a || coef[G + cap + i] != (int16_t)0x5a5a || qt[i] != 0xa5a5 || qt[G + 256 + i] != 0xa5a5) {
                fprintf(stderr, "%s %lld: guard word overwritten\n", what, arg);
                ++failures;
                break;
            }
        free(coef);
        free(qt);
    }
    rc == 0 ? ++accepted : ++refused;
    free(d);
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s <file to truncate> <file to corrupt>\n", argv[0]); return 2; }
    const std::vector<unsigned char> a = read_file(argv[1]), b = read_file(argv[2]);
    run(a.data(), a.size(), -1, "whole", 0);
    run(b.data(), b.size(), -1, "whole", 1);
    if (refused != 0) { fprintf(stderr, "an intact file was refused\n"); return 1; }
    for (size_t n = 0; n < a.size(); ++n) run(a.data(), n, -1, "truncated to", (long long)n);
    run(b.data(), b.size(), 0, "capacity", 0);
    run(b.data(), b.size(), 64, "capacity", 64);
    unsigned long long s = 0x9e3779b97f4a7c15ull;      // seeded: the same 200 corruptions every run
    std::vector<unsigned char> c;
    for (int k = 0; k < 200; ++k) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const size_t at = (size_t)((s >> 33) % b.size());
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const unsigned char v = (unsigned char)(s >> 40);
        c = b;
        c[at] = c[at] == v ? (unsigned char)(v ^ 0xff) : v;
        run(c.data(), c.size(), -1, "corruption", k);
    }
    printf("jpeg_fuzz_host: %d decoded, %d refused with a message, %d failures\n", accepted, refused, failures);
    return failures ? 1 : 0;
}
