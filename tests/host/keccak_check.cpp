// tests/host/keccak_check.cpp -- host_keccak.hpp alone, as a stand-alone program (tests/test_keccak_reading.py builds it with
// AddressSanitizer + UBSan and runs it as a child process): the two known answers of Keccak-256, the block-boundary lengths against a
// second, byte-wise sponge written here, and the packing of a digest into four words and back.  Exit status 0 = all equal.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "host_keccak.hpp"

static int failures = 0;

static void expect(bool ok, const char* what, size_t k) {
    if (ok) return;
    failures++;
    printf("MISMATCH %s at %zu\n", what, k);
}

static void hex(const uint8_t* b, size_t n, char* out) {
    for (size_t i = 0; i < n; i++) sprintf(out + 2 * i, "%02x", b[i]);
}

// the sponge byte by byte over a padded copy of the message: another route to the same function
static void keccak256_bytes(const std::vector<uint8_t>& msg, uint8_t out[32]) {
    std::vector<uint8_t> m(msg);
    const size_t pad = 136 - m.size() % 136;
    m.resize(m.size() + pad, 0);
    m[msg.size()] ^= 0x01;
    m[m.size() - 1] ^= 0x80;
    uint64_t s[25] = {0};
    for (size_t off = 0; off < m.size(); off += 136) {
        for (size_t i = 0; i < 136; i++) s[i / 8] ^= (uint64_t)m[off + i] << (8 * (i % 8));
        keccak::f1600(s);
    }
    for (int i = 0; i < 32; i++) out[i] = (uint8_t)(s[i / 8] >> (8 * (i % 8)));
}

int main() {
    uint8_t d[32];
    char h[65];
    keccak::keccak256(nullptr, 0, d);
    hex(d, 32, h);
    expect(!strcmp(h, "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"), "keccak256(\"\")", 0);
    keccak::keccak256(reinterpret_cast<const uint8_t*>("abc"), 3, d);
    hex(d, 32, h);
    expect(!strcmp(h, "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"), "keccak256(\"abc\")", 3);

    const size_t lengths[] = {0, 1, 135, 136, 137, 271, 272, 273};
    for (size_t len : lengths) {
        std::vector<uint8_t> msg(len);
        for (size_t i = 0; i < len; i++) msg[i] = (uint8_t)(31 * i + 7 * len + 1);
        uint8_t want[32];
        keccak256_bytes(msg, want);
        keccak::keccak256(len ? msg.data() : nullptr, len, d);      // an exact-size buffer: a read past it is the sanitizer's to find
        expect(!memcmp(d, want, 32), "keccak256 against the byte-wise sponge, length", len);
    }

    // hash_or_noop of n elements = keccak256 of their canonical bytes (n >= 4), the bytes themselves re-cut below that
    const size_t counts[] = {1, 3, 4, 16, 17, 18, 34, 35};
    for (size_t n : counts) {
        std::vector<uint64_t> e(n);
        for (size_t i = 0; i < n; i++) e[i] = i % 3 == 0 ? keccak::GL_P + i : i % 3 == 1 ? 0xfffffffffffffffeULL - i : 0x0123456789abcdefULL * (i + 1);
        std::vector<uint8_t> bytes(8 * n);
        for (size_t i = 0; i < n; i++) {
            const uint64_t c = keccak::canon(e[i]);
            for (int b = 0; b < 8; b++) bytes[8 * i + b] = (uint8_t)(c >> (8 * b));
        }
        uint8_t full[32] = {0};
        if (n >= 4) keccak256_bytes(bytes, full);
        else memcpy(full, bytes.data(), 8 * n);
        uint64_t got[4], l[4];
        keccak::hash_or_noop(e.data(), n, got);
        keccak::unpack25(got, l);
        uint8_t back[32] = {0};
        for (int i = 0; i < 25; i++) back[i] = (uint8_t)(l[i / 8] >> (8 * (i % 8)));
        expect(!memcmp(back, full, 25), "hash_or_noop, elements", n);
        for (int k = 0; k < 4; k++) expect(keccak::word_in_range(got[k], k), "digest word in range, elements", n);
    }

    // two_to_one of two all-ones digests = keccak256 of fifty 0xff bytes
    {
        const uint64_t ones[4] = {(1ULL << 56) - 1, (1ULL << 56) - 1, (1ULL << 56) - 1, (1ULL << 32) - 1};
        std::vector<uint8_t> msg(50, 0xff);
        uint8_t full[32];
        keccak256_bytes(msg, full);
        uint64_t got[4], l[4];
        keccak::two_to_one(ones, ones, got);
        keccak::unpack25(got, l);
        uint8_t back[32] = {0};
        for (int i = 0; i < 25; i++) back[i] = (uint8_t)(l[i / 8] >> (8 * (i % 8)));
        expect(!memcmp(back, full, 25), "two_to_one of all-ones digests", 50);
        expect(!keccak::word_in_range(1ULL << 56, 0) && !keccak::word_in_range(1ULL << 32, 3) && keccak::word_in_range(1ULL << 32, 2), "word ranges", 0);
    }
    if (failures) return 1;
    printf("keccak_check ok\n");
    return 0;
}
