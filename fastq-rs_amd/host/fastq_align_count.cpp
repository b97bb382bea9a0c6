// fastq_align_count — the GPU-backed twin of the reference's examples/alignment_count.rs: prints the number of records whose
// Smith-Waterman-Gotoh local alignment score of seq() against the Illumina adapter is above a threshold (path argument, "-"
// or nothing = stdin; plain, gzip, bzip2, xz, zstd or lz4 input, sniffed as parse_path does).  On a malformed file it fails
// like the example's `.expect("Invalid fastq file")` with the reference's error message (parallel_each's wording) and exit
// status 101.
//   --adapter SEQ --match M --mismatch X --gap-open O --gap-extend E --threshold T
//                     the alignment (fqh_align_scores); defaults: the example's adapter, 1, 0, 8, 1, 10
//   --piece-mib P     the input goes through the device in pieces of P MiB (default 256): each piece is scanned with the
//                     carry of the one before (fqh_scan), indexed (fqh_index_records) and scored (fqh_align_scores); the
//                     bytes after its last complete record go in front of the next piece, as src/buffer.rs:51-72 keeps them
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fastq.hpp"

namespace {

// Records are at most BUFSIZE bytes (a longer one is "too long" wherever it starts), so the record in progress at a cut fits
// a lead area of this size in front of every piece.
constexpr uint64_t LEAD = 2 * fastq::BUFSIZE;

struct Args {
    std::string adapter = "AATGATACGGCGACCACCGAGATCTACACTCTTTCCCTACACGACGCTCTTCCGATCT";  // examples/alignment_count.rs:8-10
    int32_t match = 1, mismatch = 0, gap_open = 8, gap_extend = 1, threshold = 10;     // ... :29-30, Identity matrix
    uint64_t piece = 256ull << 20;
};

struct Device {
    fqh_ctx *ctx = nullptr;
    void *buf = nullptr, *index = nullptr, *count = nullptr;
    ~Device() {
        if (buf) fqh_dev_free(ctx, buf);
        if (index) fqh_dev_free(ctx, index);
        if (count) fqh_dev_free(ctx, count);
        if (ctx) fqh_destroy(ctx);
    }
};

[[noreturn]] void die(const Device &d, const char *what) {
    fprintf(stderr, "%s: %s\n", what, d.ctx ? fqh_last_error(d.ctx) : "");
    exit(2);
}

uint64_t count_hits(fastq::DynReader &in, const Args &a) {
    Device d;
    if (fqh_create(0, &d.ctx) != FQH_OK) die(d, "fqh_create");
    const uint64_t piece = (a.piece + 15) & ~15ull;
    if (fqh_dev_alloc(d.ctx, LEAD + piece, &d.buf) != FQH_OK) die(d, "fqh_dev_alloc");
    if (fqh_dev_alloc(d.ctx, 8, &d.count) != FQH_OK || fqh_memset(d.ctx, d.count, 0, 8) != FQH_OK) die(d, "fqh_dev_alloc");
    uint64_t index_cap = 0;
    std::vector<uint8_t> host(LEAD + piece);
    uint8_t *const h_piece = host.data() + LEAD;
    uint8_t *const d_piece = (uint8_t *)d.buf + LEAD;
    fqh_carry carry{};
    uint64_t tail = 0;
    for (bool fin = false; !fin;) {
        uint64_t got = 0;
        while (got < piece) {
            const size_t k = in.read(h_piece + got, (size_t)(piece - got));
            if (!k) { fin = true; break; }
            got += k;
        }
        // the tail of the previous piece and this piece, contiguous, to the same place on the device
        if (tail + got && fqh_memcpy_h2d(d.ctx, d_piece - tail, h_piece - tail, tail + got) != FQH_OK) die(d, "fqh_memcpy_h2d");
        fqh_summary s;
        fqh_carry next;
        const fqh_status st = fqh_scan(d.ctx, d_piece, got, fin ? 1 : 0, &carry, nullptr, 0, &s, &next);
        if (st != FQH_OK) die(d, "fqh_scan");
        if (s.parse_status != FQH_OK) throw fastq::Error(fastq::ErrorKind::InvalidData, fastq::detail::message(s.parse_status, true));
        if (s.n_records > index_cap) {
            if (d.index) fqh_dev_free(d.ctx, d.index);
            d.index = nullptr;
            index_cap = s.n_records + s.n_records / 4;
            if (fqh_dev_alloc(d.ctx, index_cap * sizeof(fqh_idx_record), &d.index) != FQH_OK) die(d, "fqh_dev_alloc");
        }
        if (s.n_records) {
            const auto *idx = (const fqh_idx_record *)d.index;
            if (fqh_index_records(d.ctx, (fqh_idx_record *)d.index, s.n_records) != FQH_OK) die(d, "fqh_index_records");
            if (fqh_align_scores(d.ctx, d_piece, got, carry.base_offset, idx, s.n_records, (const uint8_t *)a.adapter.data(),
                                 (uint32_t)a.adapter.size(), a.match, a.mismatch, a.gap_open, a.gap_extend, a.threshold,
                                 nullptr, nullptr, nullptr, (uint64_t *)d.count) != FQH_OK)
                die(d, "fqh_align_scores");
        }
        if (!fin) {
            // no record is longer than BUFSIZE: a longer tail is a record the reference rejects wherever it lies
            if (s.tail_len > fastq::BUFSIZE)
                throw fastq::Error(fastq::ErrorKind::InvalidData, fastq::detail::message(FQH_E_TOO_LONG, true));
            tail = s.tail_len;
            memmove(h_piece - tail, h_piece + got - tail, tail);  // Buffer::clean, src/buffer.rs:51-72
        }
        carry = next;
    }
    uint64_t hits = 0;
    if (fqh_sync(d.ctx) != FQH_OK || fqh_memcpy_d2h(d.ctx, &hits, d.count, 8) != FQH_OK) die(d, "fqh_memcpy_d2h");
    return hits;
}

}  // namespace

int main(int argc, char **argv) {
    std::optional<std::string> path;
    Args a;
    for (int i = 1; i < argc; ++i) {
        const bool more = i + 1 < argc;
        if (!strcmp(argv[i], "--adapter") && more) a.adapter = argv[++i];
        else if (!strcmp(argv[i], "--match") && more) a.match = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--mismatch") && more) a.mismatch = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--gap-open") && more) a.gap_open = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--gap-extend") && more) a.gap_extend = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--threshold") && more) a.threshold = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--piece-mib") && more) a.piece = (uint64_t)std::max(1, atoi(argv[++i])) << 20;
        else path = argv[i];
    }
    if (a.adapter.empty() || a.adapter.size() > FQH_ALIGN_MAX_QUERY) {
        fprintf(stderr, "--adapter: 1 to %d bytes\n", FQH_ALIGN_MAX_QUERY);
        return 2;
    }
    uint64_t hits = 0;
    try {
        hits = fastq::with_plain_reader(path, [&](fastq::DynReader &in) { return count_hits(in, a); },
                                        std::max(1u, std::min(8u, std::thread::hardware_concurrency() / 8u)));
    } catch (const fastq::Error &e) {
        fprintf(stderr, "Invalid fastq file: %s\n", e.what());
        return 101;  // a Rust panic exits with 101
    }
    printf("%llu\n", (unsigned long long)hits);
    return 0;
}
