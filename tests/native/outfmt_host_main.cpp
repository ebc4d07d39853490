// Stand-alone run of the harness of tests/native/outfmt_host.cpp for the host sanitizers (a program of its own: nothing is
// preloaded).  With a file argument it plays the plans `python tests/outfmt_cases.py <file>` dumped (the cases of the test
// suite); without one it plays plans made here.  Every plan goes through every chunking and is compared with a serial
// restatement; every array is an exact-size heap allocation, so a read or write past an end is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

extern "C" int64_t of_host_format(const int64_t *rec_off, const int64_t *hdr_off, const int64_t *seg_first, const int64_t *seg_base,
                                  const int64_t *seg_src, const uint32_t *seg_flags, const uint8_t *hdr, const uint8_t *contig,
                                  const uint8_t *cons, int64_t nrec, int64_t nseg, int32_t width, int64_t chunk, uint8_t *out);

struct PlanData {
    std::vector<int64_t> rec_off, hdr_off, seg_first, seg_base, seg_src;
    std::vector<uint32_t> seg_flags;
    std::vector<uint8_t> hdr, contig, cons;
    int32_t width = 0;
};

// the plan as text, base by base (the rules of dh_outfmt.h restated serially)
static std::string serial(const PlanData &p)
{
    std::string s;
    const char *low = "acgtn", *up = "ACGTN";
    for (size_t r = 0; r + 1 < p.hdr_off.size(); r++) {
        s.append((const char *)p.hdr.data() + p.hdr_off[r], (size_t)(p.hdr_off[r + 1] - p.hdr_off[r]));
        int64_t col = 0, nb = 0;
        for (int64_t g = p.seg_first[r]; g < p.seg_first[r + 1]; g++) {
            const uint32_t fl = p.seg_flags[(size_t)g];
            for (int64_t k = 0; k < p.seg_base[(size_t)g + 1] - p.seg_base[(size_t)g]; k++) {
                uint32_t code = 4;
                if ((fl & 3) != 1) {
                    const std::vector<uint8_t> &buf = (fl & 3) == 0 ? p.contig : p.cons;
                    code = buf[(size_t)(p.seg_src[(size_t)g] + ((fl & 4) ? -k : k))];
                    if ((fl & 4) && code < 4) code = 3 - code;
                }
                s.push_back(((fl & 8) ? up : low)[code < 4 ? code : 4]);
                nb++;
                if (p.width > 0 && ++col == p.width) {
                    s.push_back('\n');
                    col = 0;
                }
            }
        }
        if (col != 0 || p.width <= 0) s.push_back('\n');
        (void)nb;
    }
    return s;
}

static int check(const PlanData &p, const char *name)
{
    const std::string want = serial(p);
    const int64_t nrec = (int64_t)p.hdr_off.size() - 1, nseg = (int64_t)p.seg_src.size();
    if ((int64_t)want.size() != p.rec_off[(size_t)nrec]) {
        fprintf(stderr, "%s: the plan's length %lld differs from the restatement's %zu\n", name, (long long)p.rec_off[(size_t)nrec], want.size());
        return 1;
    }
    std::vector<int64_t> chunks = {64, 112, 4096, 1 << 28};
    for (size_t r = 1; r + 1 < p.rec_off.size(); r++)
        if (p.rec_off[r] >= 64 && p.rec_off[r] % 16 == 0) {  // a chunk that ends exactly on a record boundary
            chunks.push_back(p.rec_off[r]);
            break;
        }
    for (int64_t chunk : chunks) {
        std::vector<uint8_t> out(want.size());
        const int64_t n = of_host_format(p.rec_off.data(), p.hdr_off.data(), p.seg_first.data(), p.seg_base.data(), p.seg_src.data(),
                                         p.seg_flags.data(), p.hdr.data(), p.contig.data(), p.cons.data(), nrec, nseg, p.width, chunk, out.data());
        if (n != (int64_t)want.size() || memcmp(out.data(), want.data(), want.size()) != 0) {
            fprintf(stderr, "%s: chunk %lld: the lanes' bytes differ (returned %lld)\n", name, (long long)chunk, (long long)n);
            return 1;
        }
    }
    return 0;
}

static uint32_t rnd(uint32_t &s)
{
    s = s * 1664525u + 1013904223u;
    return s >> 8;
}

// a plan of `nrec` records with random segments of every kind over random buffers
static PlanData synthetic(uint32_t seed, int32_t width, int nrec, int max_seg_len)
{
    PlanData p;
    p.width = width;
    p.contig.resize(5000);
    p.cons.resize(700);
    for (auto &b : p.contig) b = (uint8_t)(rnd(seed) % 5);
    for (auto &b : p.cons) b = (uint8_t)(rnd(seed) % 4);
    p.hdr_off.push_back(0);
    p.seg_base.push_back(0);
    p.rec_off.push_back(0);
    for (int r = 0; r < nrec; r++) {
        std::string h = ">rec" + std::to_string(r) + std::string(rnd(seed) % 90, 'x') + "\n";
        p.hdr.insert(p.hdr.end(), h.begin(), h.end());
        p.hdr_off.push_back((int64_t)p.hdr.size());
        p.seg_first.push_back((int64_t)p.seg_src.size());
        const int nsegs = (int)(rnd(seed) % 4);
        int64_t nb = 0;
        for (int g = 0; g < nsegs; g++) {
            const uint32_t kind = rnd(seed) % 3, rev = (rnd(seed) & 1) ? 4u : 0u, upper = (rnd(seed) & 1) ? 8u : 0u;
            const int64_t buf_len = kind == 0 ? (int64_t)p.contig.size() : (int64_t)p.cons.size();
            const int64_t len = 1 + rnd(seed) % std::min<int64_t>(max_seg_len, buf_len);
            const int64_t lo = rnd(seed) % (buf_len - len + 1);
            p.seg_src.push_back(kind == 1 ? 0 : (rev ? lo + len - 1 : lo));
            p.seg_flags.push_back(kind | (kind == 1 ? 0u : rev) | upper);
            p.seg_base.push_back(p.seg_base.back() + len);
            nb += len;
        }
        const int64_t body = width <= 0 ? nb + 1 : (nb == 0 ? 0 : nb + (nb + width - 1) / width);
        p.rec_off.push_back(p.rec_off.back() + (int64_t)h.size() + body);
    }
    p.seg_first.push_back((int64_t)p.seg_src.size());
    return p;
}

template <class T>
static bool rd(FILE *f, std::vector<T> &v)
{
    int64_t n = 0;
    if (fread(&n, 8, 1, f) != 1 || n < 0) return false;
    v.resize((size_t)n);
    return n == 0 || fread(v.data(), sizeof(T), (size_t)n, f) == (size_t)n;
}

int main(int argc, char **argv)
{
    int bad = 0, n = 0;
    if (argc > 1) {
        FILE *f = fopen(argv[1], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[1]);
            return 2;
        }
        int64_t ncases = 0;
        if (fread(&ncases, 8, 1, f) != 1) return 2;
        for (int64_t c = 0; c < ncases; c++) {
            PlanData p;
            int64_t w = 0;
            if (fread(&w, 8, 1, f) != 1 || !rd(f, p.rec_off) || !rd(f, p.hdr_off) || !rd(f, p.seg_first) || !rd(f, p.seg_base) ||
                !rd(f, p.seg_src) || !rd(f, p.seg_flags) || !rd(f, p.hdr) || !rd(f, p.contig) || !rd(f, p.cons)) {
                fprintf(stderr, "%s: truncated\n", argv[1]);
                return 2;
            }
            p.width = (int32_t)w;
            bad += check(p, ("case " + std::to_string(c)).c_str());
            n++;
        }
        fclose(f);
    } else {
        const int32_t widths[] = {0, 1, 3, 7, 50};
        uint32_t seed = 1;
        for (int32_t w : widths)
            for (int shape = 0; shape < 3; shape++) {
                const PlanData p = synthetic(seed++, w, shape == 0 ? 300 : 40, shape == 0 ? 5 : (shape == 1 ? 60 : 5000));
                bad += check(p, ("synthetic width " + std::to_string(w) + " shape " + std::to_string(shape)).c_str());
                n++;
            }
    }
    printf("%d plan(s), %d failed\n", n, bad);
    return bad ? 1 : 0;
}
