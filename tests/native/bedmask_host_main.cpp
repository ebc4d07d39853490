// Stand-alone run of the BED parser (dentist_amd/csrc/dh_bedmask.cpp) and of the track extras of a mask
// (dentist_amd/csrc/dazzdb.cpp) for the host sanitizers (a program of its own: nothing is preloaded).  Both are host code of the
// library and are compiled into this program as they are; what they need of the rest of the library (dh_fail, dh_last_error) is
// defined here.  The BED texts are generated: well-formed ones are compared with a restatement of the rules, malformed ones
// (every prefix of a text, oversized numbers, empty fields, broken data comments) must be refused or accepted, never overrun --
// every text is an exact-size heap allocation without a NUL behind it.  The extras of a mask are read back from a file cut at
// every byte.  Files go to a directory of their own under $TMPDIR (or /tmp), removed at the end.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../../include/dentist_hip.h"

static std::string g_err;
int dh_fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}
extern "C" const char *dh_last_error(void) { return g_err.c_str(); }

static int g_failures = 0;
#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            fprintf(stderr, "FAILED %s: ", #cond); \
            fprintf(stderr, __VA_ARGS__);      \
            fprintf(stderr, "\n");             \
            g_failures++;                      \
        }                                      \
    } while (0)

// scafA: three contigs with runs of n between them; scafB: one contig
static const int kLen[3] = {100, 80, 60}, kGap[2] = {20, 30};
static const int kBegin[3] = {0, 120, 230};

struct Want {
    int32_t contig, begin, end;
    int64_t a, b;
    std::vector<int64_t> reads;
};

// dh_bed_to_mask on an exact-size copy of `text`
static int parse(const dh_dazz *db, const std::string &text, int data_comments, dh_bed_mask **out)
{
    char *exact = new char[text.size() ? text.size() : 1];
    memcpy(exact, text.data(), text.size());
    const int rc = dh_bed_to_mask(db, exact, (int64_t)text.size(), "generated.bed", data_comments, out);
    delete[] exact;
    return rc;
}

static void well_formed(const dh_dazz *db, std::mt19937 &rng, int round)
{
    // ascending intervals of scafA, then one of scafB
    std::string text;
    std::vector<Want> want;
    int pos = (int)(rng() % 40);
    int64_t next_id = 1;
    while (pos < 290) {
        const int begin = pos, end = std::min(begin + 1 + (int)(rng() % 90), 400);
        std::vector<Want> mine;
        for (int c = 0; c < 3; c++) {
            const int cb = kBegin[c], ce = kBegin[c] + kLen[c];
            if (ce <= begin || cb >= end) continue;
            mine.push_back(Want{c, std::max(begin, cb) - cb, std::min(end, ce) - cb, 0, 0, {}});
        }
        pos = end + (int)(rng() % 30);
        if (mine.empty()) continue;  // (inside a run of n: refused, tried below)
        const int64_t a = next_id++, b = next_id++;
        std::vector<int64_t> reads;
        for (unsigned k = rng() % 4; k > 0; k--) reads.push_back((int64_t)(rng() % 100000));
        text += "scafA\t" + std::to_string(begin) + "\t" + std::to_string(end) + "\t";
        if (rng() % 3 == 0) text += "reads-1-2-3|";  // overwritten by the later part
        if (rng() % 3 == 0) text += "note-x-y|";
        text += "contigs-" + std::to_string(a) + "-" + std::to_string(b) + "|reads";
        for (int64_t r : reads) text += "-" + std::to_string(r);
        text += rng() % 4 == 0 ? "\n\n" : "\n";
        for (Want &w : mine) {
            w.a = a, w.b = b, w.reads = reads;
            want.push_back(w);
        }
    }
    text += "scafB\t3\t9\tcontigs-7-8";
    if (round % 2) text += "\n";
    want.push_back(Want{3, 3, 9, 7, 8, {}});
    dh_bed_mask *m = nullptr;
    const int rc = parse(db, text, 1, &m);
    EXPECT(rc == DH_OK, "round %d: %s", round, dh_last_error());
    if (rc != DH_OK) return;
    EXPECT(dh_bed_mask_count(m) == (int64_t)want.size() && dh_bed_mask_ncontigs(m) == 4, "round %d: %lld intervals", round, (long long)dh_bed_mask_count(m));
    if (dh_bed_mask_count(m) == (int64_t)want.size()) {
        const int64_t *ptr = dh_bed_mask_ptr(m), *ids = dh_bed_mask_contig_ids(m), *off = dh_bed_mask_read_off(m), *rd = dh_bed_mask_read_ids(m);
        const int32_t *iv = dh_bed_mask_iv(m);
        for (size_t i = 0; i < want.size(); i++) {
            const Want &w = want[i];
            EXPECT(ptr[w.contig] <= (int64_t)i && (int64_t)i < ptr[w.contig + 1], "round %d interval %zu: contig", round, i);
            EXPECT(iv[2 * i] == w.begin && iv[2 * i + 1] == w.end && ids[2 * i] == w.a && ids[2 * i + 1] == w.b, "round %d interval %zu", round, i);
            EXPECT(off[i + 1] - off[i] == (int64_t)w.reads.size() && std::equal(w.reads.begin(), w.reads.end(), rd + off[i]), "round %d interval %zu: reads",
                   round, i);
        }
    }
    dh_bed_mask_destroy(m);
    // every prefix of the text, with and without data comments: accepted or refused, and a refusal names the file
    for (size_t cut = 0; cut < text.size(); cut++)
        for (int dc = 0; dc < 2; dc++) {
            m = nullptr;
            const int prc = parse(db, text.substr(0, cut), dc, &m);
            EXPECT(prc == DH_OK || (prc == DH_EINVAL && strstr(dh_last_error(), "generated.bed:")), "round %d prefix %zu: %d %s", round, cut, prc,
                   dh_last_error());
            dh_bed_mask_destroy(m);
        }
}

static void malformed(const dh_dazz *db)
{
    const char *const big = "99999999999999999999999999999999999999";
    const std::string lines[] = {
        "scafA", "scafA\t", "scafA\t\t", "scafA\t\t\t", "\t\t\t", "\t", "scafA\t1", "scafA\t1\t", "scafA\t\t2", std::string("scafA\t1\t") + big,
        std::string("scafA\t") + big + "\t5", "scafA\t2147483647\t2147483647", "scafA\t2147483648\t2147483649", "scafA\t-1\t5", "scafA\t+1\t5",
        "scafA\t 1\t5", "scafA\t1 \t5", "scafA\t0x1\t5", "scafA\t5\t4", "scafA\t100\t120", "scafA\t290\t291", "scafA\t0\t0", "nowhere\t1\t2",
        "scafA\tsome more words\t1\t2", "scafA\t1\t2", "scafA\t1\t2\t", "scafA\t1\t2\t|", "scafA\t1\t2\t||||", "scafA\t1\t2\t-", "scafA\t1\t2\t-|-",
        "scafA\t1\t2\tcontigs", "scafA\t1\t2\tcontigs-", "scafA\t1\t2\tcontigs--", "scafA\t1\t2\tcontigs---", "scafA\t1\t2\tcontigs-1", "scafA\t1\t2\tcontigs-1-",
        "scafA\t1\t2\tcontigs-1-2-3", "scafA\t1\t2\tcontigs-a-2", "scafA\t1\t2\tcontigs-1-2|reads-", "scafA\t1\t2\tcontigs-1-2|reads--",
        "scafA\t1\t2\tcontigs-1-2|reads-x", std::string("scafA\t1\t2\tcontigs-1-") + big, std::string("scafA\t1\t2\tcontigs-1-2|reads-") + big,
        "scafA\t1\t2\tcontigs-4294967295-4294967296", "scafA\t1\t2\treads-1", "scafA\t1\t2\tcontigs-1-2|contigs-3", "scafA\t1\t2\tcontigs-1-2\tmore\tcolumns",
        "scafA\t1\t2\tcontigs-1-2\r", "scafA\t30\t40\tcontigs-1-2\nscafA\t10\t20\tcontigs-1-2", "scafB\t1\t2\tcontigs-1-2\nscafA\t1\t2\tcontigs-1-2",
        std::string("scafA\t1\t2\tcontigs-1-2|reads\0-1", 30)};
    int refused = 0, accepted = 0;
    for (const std::string &l : lines)
        for (int dc = 0; dc < 2; dc++)
            for (const char *tail : {"", "\n", "\n\n"}) {
                dh_bed_mask *m = nullptr;
                const int rc = parse(db, l + tail, dc, &m);
                EXPECT(rc == DH_OK || (rc == DH_EINVAL && strstr(dh_last_error(), "generated.bed:")), "`%s`: %d %s", l.c_str(), rc, dh_last_error());
                EXPECT((rc == DH_OK) == (m != nullptr), "`%s`: a handle and a failure", l.c_str());
                (rc == DH_OK ? accepted : refused)++;
                dh_bed_mask_destroy(m);
            }
    EXPECT(refused > 100 && accepted > 20, "%d refused, %d accepted", refused, accepted);
}

static std::string slurp(const std::string &path)
{
    std::string s;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return s;
    char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, got);
    fclose(f);
    return s;
}

static void extras_cut_at_every_byte(const std::string &dir, const std::string &dam)
{
    const int64_t ptr[5] = {0, 1, 1, 2, 2};
    const int32_t iv[4] = {5, 9, 1, 2};
    const int64_t ints[5] = {1, -2, 3, int64_t(1) << 40, 5};
    const double reals[3] = {0.5, -1.25, 1e300};
    EXPECT(dh_dazz_write_mask(dam.c_str(), "m", 4, ptr, iv) == DH_OK, "%s", dh_last_error());
    EXPECT(dh_dazz_write_extra(dam.c_str(), "m", "contigs", DH_EXTRA_INT64, DH_ACCUM_EXACT, ints, 5) == DH_OK, "%s", dh_last_error());
    EXPECT(dh_dazz_write_extra(dam.c_str(), "m", "", DH_EXTRA_INT64, DH_ACCUM_SUM, nullptr, 0) == DH_OK, "%s", dh_last_error());
    EXPECT(dh_dazz_write_extra(dam.c_str(), "m", "weights", DH_EXTRA_DOUBLE, DH_ACCUM_SUM, reals, 3) == DH_OK, "%s", dh_last_error());
    const std::string anno = dir + "/.ref.m.anno", whole = slurp(anno);
    const size_t mask_end = 8 + 8 * 5, first_end = mask_end + 16 + 7 + 40, second_end = first_end + 16;
    EXPECT(whole.size() == second_end + 16 + 7 + 24, "%zu bytes", whole.size());
    const size_t start[4] = {mask_end, first_end, second_end, whole.size()};
    const char *const names[3] = {"contigs", "", "weights"};
    const int64_t counts[3] = {5, 0, 3};
    for (size_t cut = 0; cut <= whole.size(); cut++) {
        FILE *f = fopen(anno.c_str(), "wb");
        if (!f || (cut && fwrite(whole.data(), 1, cut, f) != cut) || fclose(f) != 0) {
            EXPECT(false, "cannot write %s", anno.c_str());
            return;
        }
        for (const char *name : {"contigs", "weights", "", "absent"}) {
            int32_t vtype = -1, accum = -1;
            const int64_t cnt = dh_dazz_read_extra(dam.c_str(), "m", name, &vtype, &accum, nullptr, 0);
            // what a file of `cut` bytes must give for this name: the extras are walked in their order, and one that is cut is
            // reported whether or not it is the one asked for
            const bool is_first = !strcmp(name, "contigs");
            int64_t expect = cut < mask_end ? DH_EINVAL : DH_ENOTFOUND;
            for (int i = 0; i < 3 && cut >= mask_end; i++) {
                if (cut == start[i]) break;
                if (cut < start[i + 1]) {
                    expect = DH_EINVAL;
                    break;
                }
                if (!strcmp(name, names[i])) {
                    expect = counts[i];
                    break;
                }
            }
            EXPECT(cnt == expect, "cut %zu name `%s`: %lld, expected %lld (%s)", cut, name, (long long)cnt, (long long)expect, dh_last_error());
            if (cnt == DH_EINVAL) EXPECT(strstr(dh_last_error(), "current extra index") != nullptr, "cut %zu: %s", cut, dh_last_error());
            if (cnt <= 0) continue;
            // filled into exact-size arrays, and into one that is too small
            for (int64_t cap : {cnt, cnt - 1}) {
                int64_t *data = new int64_t[(size_t)std::max<int64_t>(cap, 1)];
                int32_t vt = vtype;
                EXPECT(dh_dazz_read_extra(dam.c_str(), "m", name, &vt, nullptr, data, cap) == cnt, "cut %zu: %s", cut, dh_last_error());
                EXPECT(memcmp(data, is_first ? (const void *)ints : (const void *)reals, (size_t)cap * 8) == 0, "cut %zu name `%s`: values", cut, name);
                delete[] data;
            }
            EXPECT(vtype == (is_first ? DH_EXTRA_INT64 : DH_EXTRA_DOUBLE) && accum == (is_first ? DH_ACCUM_EXACT : DH_ACCUM_SUM), "cut %zu: type and mode", cut);
            int32_t wrong = is_first ? DH_EXTRA_DOUBLE : DH_EXTRA_INT64;
            EXPECT(dh_dazz_read_extra(dam.c_str(), "m", name, &wrong, nullptr, nullptr, 0) == DH_EINVAL, "cut %zu: the wrong vtype was accepted", cut);
        }
    }
    // headers that lie: a negative length, a name longer than the file, data longer than the file
    for (int field : {1, 3})
        for (int32_t value : {-1, INT32_MAX, INT32_MIN, 1 << 20}) {
            std::string bad = whole;
            memcpy(&bad[mask_end + 4 * (size_t)field], &value, 4);
            FILE *f = fopen(anno.c_str(), "wb");
            if (!f || fwrite(bad.data(), 1, bad.size(), f) != bad.size() || fclose(f) != 0) {
                EXPECT(false, "cannot write %s", anno.c_str());
                return;
            }
            int32_t vtype = -1;
            EXPECT(dh_dazz_read_extra(dam.c_str(), "m", "weights", &vtype, nullptr, nullptr, 0) == DH_EINVAL, "field %d = %d was accepted", field, value);
        }
}

int main()
{
    const char *tmp = getenv("TMPDIR");
    std::string dir = std::string(tmp && *tmp ? tmp : "/tmp") + "/bedmask_host_XXXXXX";
    if (!mkdtemp(&dir[0])) {
        perror("mkdtemp");
        return 2;
    }
    const std::string dam = dir + "/ref.dam";
    std::mt19937 rng(12345);
    auto bases = [&](int n) {
        std::string s;
        for (int i = 0; i < n; i++) s.push_back("acgt"[rng() % 4]);
        return s;
    };
    const std::string fasta = ">scafA\tsome more words\n" + bases(kLen[0]) + std::string((size_t)kGap[0], 'n') + bases(kLen[1]) + std::string((size_t)kGap[1], 'n') +
                              bases(kLen[2]) + "\n>scafB\n" + bases(90) + "\n";
    dh_dazz *db = nullptr;
    if (dh_dazz_create_dam(dam.c_str(), fasta.data(), (int64_t)fasta.size()) || dh_dazz_split(dam.c_str(), 20, 1, 200) || dh_dazz_open(dam.c_str(), &db)) {
        fprintf(stderr, "cannot make the .dam: %s\n", dh_last_error());
        return 2;
    }
    EXPECT(dh_dazz_nreads(db) == 4 && dh_dazz_fpulse(db)[1] == kBegin[1] && dh_dazz_fpulse(db)[2] == kBegin[2], "the contigs of the .dam");
    for (int round = 0; round < 200; round++) well_formed(db, rng, round);
    malformed(db);
    extras_cut_at_every_byte(dir, dam);
    dh_dazz_close(db);
    dh_dazz_remove(dam.c_str());
    rmdir(dir.c_str());
    if (g_failures) {
        fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    printf("bedmask_host_san: ok\n");
    return 0;
}
