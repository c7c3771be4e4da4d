// Host-side execution of what the wire-import kernels run per entry and per row (acvm_amd/csrc/wire_decode.hpp is __host__ __device__).
// The tool judges nothing: it answers the commands on its standard input, one line each, and tests/test_wire_decode_on_host.py compares the
// answers with bytes.fromhex, int, zlib.crc32 and tests/wire_ref.py.
//   unhex4 DWORD              four characters as a decimal dword -> NIBBLES BAD (both decimal; BAD has bit 7 of every byte that is no hex digit)
//   unhex CHARS               CHARS: 64 bytes as hex -> VALID and the 32 bytes lo, hi spell in memory order, as hex
//   value CHARS               -> VALID, then the canonical value (reduced mod p), the row and the plane word import_decode gives for lo / hi, as
//                             8 little-endian limbs each in hex, least significant first
//   count CONTAINER PITCH N_INITIAL N HAVE_LENGTH LENGTH   -> READABLE OK
//   frame N                   -> the trailer's offset, the ISIZE word, the joint offsets of a GZIP_STORED row of N entries
//   crc BODY                  BODY: a canonical body as hex -> the CRC-32 its trailer must hold, accumulated entry by entry as the kernel does
//   key INSTANCE CLASS RANK RANK_BITS   -> the key as decimal and the three fields read back from it
//   position KEY N { ID } x N -> the position of KEY among the ids (in the order given), or 4294967295
#include "../acvm_amd/csrc/wire_decode.hpp"
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>
using namespace acvm;

static bool read_hex(std::vector<uint8_t> &out) {
    static char buf[1 << 20];
    if (scanf("%1048575s", buf) != 1) return false;
    const size_t n = strlen(buf);
    if (n % 2) return false;
    out.resize(n / 2);
    for (size_t i = 0; i < out.size(); i++) {
        unsigned v = 0;
        if (sscanf(buf + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}
static void print_fr(const Fr &x) {
    for (int k = 0; k < 8; k++) printf(" %08x", x.v[k]);
}

int main() {
    std::unique_ptr<uint32_t[]> sliced(new uint32_t[WIRE_CRC_SLICED_WORDS]);  // exactly this many on the heap: a lookup past the end is one the sanitizer sees
    for (uint32_t k = 0; k < WIRE_CRC_SLICED_WORDS; k++) sliced[k] = wire_crc_sliced_entry(k);
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "unhex4")) {
            uint32_t chars = 0, bad = 0;
            if (scanf("%u", &chars) != 1) return 2;
            const uint32_t nibbles = wire_unhex4(chars, bad);
            printf("%u %u\n", nibbles, bad);
        } else if (!strcmp(cmd, "unhex") || !strcmp(cmd, "value")) {
            std::vector<uint8_t> raw;
            if (!read_hex(raw) || raw.size() != 64) return 2;
            uint32_t chars[16];
            memcpy(chars, raw.data(), 64);
            uint4 lo, hi;
            const bool valid = wire_unhex(chars, lo, hi);
            if (cmd[0] == 'u') {
                uint8_t bytes[32];
                memcpy(bytes, &lo, 16);
                memcpy(bytes + 16, &hi, 16);
                printf("%d ", (int)valid);
                for (int k = 0; k < 32; k++) printf("%02x", bytes[k]);
                printf("\n");
            } else {
                const ImportDecoded d = import_decode(lo, hi, EXPORT_ENC_BE32);
                printf("%d", (int)valid);
                print_fr(d.canonical);
                print_fr(d.row);
                printf(" %08x\n", d.plane);
            }
        } else if (!strcmp(cmd, "count")) {
            uint32_t container = 0, n_initial = 0, have = 0;
            uint64_t pitch = 0, n = 0, length = 0;
            if (scanf("%u %" SCNu64 " %u %" SCNu64 " %u %" SCNu64, &container, &pitch, &n_initial, &n, &have, &length) != 6) return 2;
            printf("%d %d\n", (int)wire_in_count_readable(container, pitch), (int)wire_in_count_ok(container, pitch, n_initial, n, have != 0, length));
        } else if (!strcmp(cmd, "frame")) {
            uint64_t n = 0;
            if (scanf("%" SCNu64, &n) != 1) return 2;
            printf("%" PRIu64 " %u", wire_in_trailer_offset(n), wire_in_isize(n));
            for (uint64_t block = 1; block < wire_blocks(wire_body_bytes(n)); block++) printf(" %" PRIu64, wire_in_joint_offset(block));
            printf("\n");
        } else if (!strcmp(cmd, "crc")) {
            std::vector<uint8_t> body;
            if (!read_hex(body) || body.size() < 8 || (body.size() - 8) % WIRE_ENTRY_BYTES) return 2;
            const uint32_t n = (uint32_t)((body.size() - 8) / WIRE_ENTRY_BYTES);
            const uint32_t step = wire_crc_xpow_bytes(WIRE_ENTRY_BYTES);
            std::vector<uint32_t> pow((size_t)n + 1);  // the plan's power table
            pow[0] = 0x80000000u;
            for (uint32_t k = 1; k <= n; k++) pow[k] = wire_crc_mul(pow[k - 1], step);
            uint32_t entries = 0;
            for (uint32_t r = 0; r < n; r++) {
                uint32_t words[WIRE_ENTRY_WORDS];
                memcpy(words, body.data() + 8 + (size_t)WIRE_ENTRY_BYTES * r, WIRE_ENTRY_BYTES);
                entries ^= wire_crc_entry(words, pow[n - 1 - r], sliced.get());
            }
            printf("%u\n", wire_in_crc(n, pow[n], wire_crc_xpow_bytes(8), entries));
        } else if (!strcmp(cmd, "key")) {
            uint64_t instance = 0;
            uint32_t cls = 0, rank = 0, bits = 0;
            if (scanf("%" SCNu64 " %u %u %u", &instance, &cls, &rank, &bits) != 4) return 2;
            const uint64_t key = wire_in_key(instance, cls, rank, bits);
            printf("%" PRIu64 " %u %u %u\n", key, wire_in_key_instance(key, bits), wire_in_key_class(key, bits), wire_in_key_rank(key, bits));
        } else if (!strcmp(cmd, "position")) {
            uint32_t key = 0, n = 0;
            if (scanf("%u %u", &key, &n) != 2) return 2;
            std::vector<uint32_t> ids(n), positions(n);
            for (uint32_t &w : ids)
                if (scanf("%u", &w) != 1) return 2;
            std::iota(positions.begin(), positions.end(), 0u);
            std::stable_sort(positions.begin(), positions.end(), [&](uint32_t x, uint32_t y) { return ids[x] < ids[y]; });
            std::unique_ptr<uint32_t[]> keys(new uint32_t[n]), pos(new uint32_t[n]);  // exactly n entries on the heap
            for (uint32_t k = 0; k < n; k++) { keys[k] = ids[positions[k]]; pos[k] = positions[k]; }
            printf("%u\n", wire_in_position(keys.get(), pos.get(), n, key));
        } else {
            fprintf(stderr, "unknown command %s\n", cmd);
            return 2;
        }
    }
    return 0;
}
