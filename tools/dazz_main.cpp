// dazz_main.cpp -- the rest of the executable boundary of DENTIST's hot path over libdentist_hip.so:
// one multi-call binary, the tool is chosen by argv[0] (or `--tool <name>` as first argument):
//
//   fasta2DB / fasta2DAM  -i <db>  (FASTA on stdin) | <db> <fasta>...   dazzler.d:6233-6330
//   DBsplit [-f] [-a] [-x<n>] [-s<mb>] <db>                             dazzler.d:6332-6345
//   DBrm <db>...                                                        dazzler.d:6115-6119
//   DBdust <db>                      writes the `dust` mask track       processPileUps/package.d:476, 655
//   DBdump [-r -h -s -i] <db> [ids | a-b]   SURVEY Appendix B grammar   dazzler.d:6445-6505, parser :2788-3078
//   DBshow [-n] <db> [ids]           FASTA / scaffold structure lines   dazzler.d:4609-4690, 6507-6517
//   LAmerge <out.las> <in.las>...                                       snakemake/Snakefile:1173-1185
//   DAScover -v <db> <las> ; DASqv -v -c<cov> <db> <las>   `qual` track dazzler.d:6142-6156
//   computeintrinsicqv -d<depth> <db> <las>             `inqual` track  dazzler.d:6172-6183
//   daccord [-t<n>] [-I<i>,<j>] [-f] [--eprofonly] <las> <db>           dazzler.d:6185-6231
//                                    consensus FASTA on stdout; --eprofonly writes <las>.eprof
//   merge-insertions <merged.db> <batch.db>...   (DENTIST's own sub-command, commands/mergeInsertions.d:42-164,
//                                    snakemake/Snakefile:1315-1334; here so that batches written by this library
//                                    can be merged without the D binary)
//   LAsplit <target with @ or #> <parts> < <source.las>     the workflow's split of a merged .las for the validation blocks
//                                    (snakemake/Snakefile:1426-1434): nearly equal parts, cut between A reads
//   Catrack [-v] [-f] [-d] <db> <track>          block mask tracks .<db>.<block>.<track>.{anno,data} concatenated into the
//                                    DB's track (snakemake/Snakefile:1111-1123; track layout dazzler.d:4943-5170)
//   TANmask [-v] [-l<int(500)>] [-n<track(tan)>] <db> <TAN las>...   self alignments of a read -> mask intervals
//                                    (snakemake/Snakefile:1095-1108); the block's track when the .las names a block
//   LApaf [-a] [-c] [-w<int(100)>] <A:db|dam> [<B:db|dam>] <align:las> [first-last]   base-level alignments of the records of a
//                                    .las as PAF with an extended cigar (dh_la_edit_paths: getExactAlignment's per-trace-point
//                                    part, dazzler.d:2405-2426); -a adds the alignment text (SequenceAlignment.toString)
//   LAtranspose [-b] <A:db|dam> <B:db|dam> <in:las> <out:las>   the same alignments with the roles of the sequences exchanged
//                                    (dh_la_transpose: the file `damapper -C` names <B>.<A>.las, dazzler.d:6158-6170, as the
//                                    exact transposition of <in>); -b sets the chain flags
//   DBnw [-f] [-a] [-w<int(100)>] <A:db|dam> <B:db|dam> [first-last]   read i of A against read i of B end to end
//                                    (dh_nw_batch: findAlignment, util/string.d:478-520; -f free shift): pair, lengths,
//                                    score, matches, columns, extended cigar; -a adds the alignment text
//   stretcher [--auto] [--stdout | --outfile=<file>] [--aformat=pair] [--awidth=<int(50)>] [--sreverse2] [--gapopen=<int(16)>]
//             [--gapextend=<int(4)>] <a:fasta> <b:fasta>   (one dash or two) the first record of each file aligned end to end
//                                    with affine gap costs (dh_nw_affine_batch), written as EMBOSS `pair` text
//                                    (dh_format_pair): the call of `dentist check-results` (commands/checkResults.d:2091-2100)
//   fm-index [-P<dir>] [-r] <reference> [<queries>...]   every exact occurrence of every query line (-r: and of its reverse
//                                    complement) in the records (lines) of <reference>, one TAB-separated line per hit
//                                    (dh_exact_locate): the reference's external/fm-index.cpp as `dentist check-results`
//                                    calls it (commands/checkResults.d:511-565, 654-687); leaves <reference>.fm9
//   chain-local-alignments [--max-indel=<bps>] [--max-chain-gap=<bps>] [--max-relative-overlap=<f>] [--min-relative-score=<f>]
//             [--min-score=<n>] <ref-db> [<reads-db>] <in:las> <out:las>   the local alignments of every (A, B) pair chained
//                                    (dh_la_chain: chainLocalAlignments, common/alignments/chaining.d:122-334): every accepted
//                                    chain as one run of records, alternate chains included -- the command of the same name
//                                    (commands/chainLocalAlignments.d; options commandline.d:945-951, 1813-2165)
//   propagate-mask -m <mask> [-m <mask>]... <ref-db> [<reads-db>] <db-alignment> <out-mask>   the union of the masks of <ref-db>
//                                    carried through the alignments to <reads-db> (to <ref-db> itself when it is omitted) and
//                                    written there as <out-mask> (dh_la_propagate_mask: `dentist propagate-mask`,
//                                    commands/propagateMask.d:136-305; snakemake/Snakefile:1218-1255)
//   validate-regions [--min-coverage-reads=<n> | --read-coverage=<f> --ploidy=<n>] [--min-spanning-reads=<n>]
//                    [--region-context=<bps>] [--weak-coverage-window=<bps>] [--weak-coverage-mask=<mask>] [--report-all]
//                    <ref-db> <reads-db> <in.las> <regions-mask>
//                                    one JSON line per invalid region (per region with --report-all) of the mask <regions-mask>
//                                    of <ref-db>, the weak-coverage mask written on request (dh_la_validate_regions: `dentist
//                                    validate-regions`, commands/validateRegions.d:141-512; snakemake/Snakefile:1425-1466)
//   collect [--mask=<name>[,<name>...]]... [--max-alignment-error=<f>] [--min-anchor-length=<n>] [--proper-alignment-allowance=<n>]
//           [--min-spanning-reads=<n>] [--best-pile-up-margin=<f>] [--existing-gap-bonus=<f>] [--no-merge-extension]
//           <ref-db> <reads-db> <ref-vs-reads.las> <pile-ups.db>
//                                    the alignments filtered on the device (dh_la_collect_filter), the scaffold graph with its
//                                    bubbles resolved, every pile-up written to <pile-ups.db> (`dentist collect`,
//                                    commands/collectPileUps/package.d:88-206; snakemake/Snakefile:1257-1290)
//   mask-repetitive-regions [--read-coverage=<f> | --max-coverage-reads=<n>] [--max-improper-coverage-reads=<n>]
//           [--max-coverage-self=<n>] [--proper-alignment-allowance=<n>] [--debug-repeat-masks] <ref-db> [<reads-db>] <db-alignment>
//           <repeat-mask>           the mask of the contig bases whose coverage by alignment chains (with <reads-db>: also by the
//                                    improper ones) leaves its bounds, written as a mask track of <ref-db>
//                                    (dh_la_repeat_mask: `dentist mask-repetitive-regions`, commands/maskRepetitiveRegions.d:
//                                    129-430, commandline.d:1840-1972)
// DENTIST only sees exit codes, files and stdout of these tools; flags it never emits are rejected.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "../include/dentist_hip.h"

static std::string g_tool;
static void die(const std::string &msg, int rc = 1)
{
    fprintf(stderr, "%s: %s\n", g_tool.c_str(), msg.c_str());
    exit(rc);
}
#define CHK(call)                                                                                 \
    do {                                                                                          \
        if (int rc_ = (call)) die(std::string(#call) + ": " + dh_last_error(), rc_ < 0 ? -rc_ : rc_); \
    } while (0)

static std::string slurp(FILE *f)
{
    std::string s;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, got);
    return s;
}
static bool is_dam(const std::string &p) { return p.size() > 4 && p.compare(p.size() - 4, 4, ".dam") == 0; }

// ---------------------------------------------------------------------------------- DB tools
static int tool_fasta2(bool dam, const std::vector<std::string> &args)
{
    bool from_stdin = false;
    std::vector<std::string> pos;
    for (const std::string &a : args) {
        if (a == "-i" || a.compare(0, 2, "-i") == 0)
            from_stdin = true;
        else if (a == "-v")
            ;
        else if (a[0] == '-')
            die("unknown option " + a);
        else
            pos.push_back(a);
    }
    if (pos.empty()) die("usage: fasta2DB|fasta2DAM [-v] <path> ( -i | <input:fasta> ... )");
    std::string text;
    if (from_stdin)
        text = slurp(stdin);
    else
        for (size_t i = 1; i < pos.size(); i++) {
            FILE *f = fopen(pos[i].c_str(), "r");
            if (!f) die("cannot open " + pos[i]);
            text += slurp(f);
            fclose(f);
            if (!text.empty() && text.back() != '\n') text += '\n';
        }
    if (dam)
        CHK(dh_dazz_create_dam(pos[0].c_str(), text.data(), (int64_t)text.size()));
    else
        CHK(dh_dazz_create_db(pos[0].c_str(), text.data(), (int64_t)text.size()));
    return 0;
}

static int tool_dbsplit(const std::vector<std::string> &args)
{
    int cutoff = 0, all = 0;
    long long size = 200;
    std::string db;
    for (const std::string &a : args) {
        if (a == "-a")
            all = 1;
        else if (a == "-f")
            ;
        else if (a.compare(0, 2, "-x") == 0)
            cutoff = atoi(a.c_str() + 2);
        else if (a.compare(0, 2, "-s") == 0)
            size = (long long)atof(a.c_str() + 2);
        else if (a[0] == '-')
            die("unknown option " + a);
        else
            db = a;
    }
    if (db.empty()) die("usage: DBsplit [-af] [-x<int>] [-s<double(200.)>] <path:db|dam>");
    CHK(dh_dazz_split(db.c_str(), cutoff, all, size));
    return 0;
}

static int tool_dbrm(const std::vector<std::string> &args)
{
    for (const std::string &a : args)
        if (a[0] != '-') CHK(dh_dazz_remove(a.c_str()));
    return 0;
}

static dh_dazz *open_dazz(const std::string &path)
{
    dh_dazz *d = nullptr;
    CHK(dh_dazz_open(path.c_str(), &d));
    return d;
}

// record numbers (1-based) from `ids` / `a-b` arguments; empty = all
static std::vector<int32_t> record_list(const std::vector<std::string> &sel, int32_t first, int32_t n)
{
    std::vector<int32_t> ids;
    if (sel.empty()) {
        for (int32_t i = 0; i < n; i++) ids.push_back(i);
        return ids;
    }
    for (const std::string &s : sel) {
        int a = 0, b = 0;
        if (sscanf(s.c_str(), "%d-%d", &a, &b) == 2)
            ;
        else if (sscanf(s.c_str(), "%d", &a) == 1)
            b = a;
        else
            die("bad record selector " + s);
        for (int x = a; x <= b; x++) {
            const int32_t loc = x - 1 - first;
            if (loc < 0 || loc >= n) die("record " + std::to_string(x) + " is not in the DB");
            ids.push_back(loc);
        }
    }
    return ids;
}

static char qv_char(int q) { return q < 26 ? (char)('a' + q) : (char)('A' + std::min(q, 50) - 26); }

static int tool_dbdump(const std::vector<std::string> &args)
{
    bool fr = false, fh = false, fs = false, fi = false;
    std::string db;
    std::vector<std::string> sel;
    for (const std::string &a : args) {
        if (a[0] == '-' && a.size() > 1 && !isdigit((unsigned char)a[1])) {
            for (size_t x = 1; x < a.size(); x++) switch (a[x]) {
                case 'r': fr = true; break;
                case 'h': fh = true; break;
                case 's': fs = true; break;
                case 'i': fi = true; break;
                case 'u': case 'U': break;
                default: die("unknown option " + a);
                }
        } else if (db.empty())
            db = a;
        else
            sel.push_back(a);
    }
    if (db.empty()) die("usage: DBdump [-rhsi] <path:db|dam> [ <reads:range> ... ]");
    dh_dazz *d = open_dazz(db);
    const int32_t n = dh_dazz_nreads(d), first = dh_dazz_first_id(d);
    const std::vector<int32_t> ids = record_list(sel, first, n);
    const int64_t *off = dh_dazz_offsets(d);
    const uint8_t *bases = dh_dazz_bases(d);
    std::vector<int64_t> qptr;
    std::vector<uint8_t> qv;
    if (fi) {
        qptr.resize((size_t)n + 1);
        const int64_t m = dh_dazz_read_track(d, db.c_str(), "qual", qptr.data(), nullptr, 0);
        if (m < 0) die(std::string("-i needs the qual track (run DASqv): ") + dh_last_error());
        qv.resize((size_t)std::max<int64_t>(m, 1));
        dh_dazz_read_track(d, db.c_str(), "qual", qptr.data(), qv.data(), m);
    }
    // header lines: totals and maxima of every line type (dazzler.d:2788-2813 reads `+ R` and `+ S`)
    int64_t tot_s = 0, max_s = 0, tot_h = 0, max_h = 0, tot_i = 0, max_i = 0;
    for (int32_t i : ids) {
        const int64_t l = off[i + 1] - off[i];
        tot_s += l;
        max_s = std::max(max_s, l);
        const int64_t hl = (int64_t)strlen(dh_dazz_header(d, i));
        tot_h += hl;
        max_h = std::max(max_h, hl);
        if (fi) {
            const int64_t ql = qptr[(size_t)i + 1] - qptr[(size_t)i];
            tot_i += ql;
            max_i = std::max(max_i, ql);
        }
    }
    printf("+ R %zu\n+ M 0\n", ids.size());
    if (fh) printf("+ H %lld\n@ H %lld\n", (long long)tot_h, (long long)max_h);
    if (fs) printf("+ S %lld\n@ S %lld\n", (long long)tot_s, (long long)max_s);
    if (fi) printf("+ I %lld\n@ I %lld\n", (long long)tot_i, (long long)max_i);
    static const char ACGT[] = "acgtn";
    const bool dam = is_dam(db) || (db.find(".db") == std::string::npos && dh_dazz_header(d, 0)[0] == '>');
    std::string seq;
    for (int32_t i : ids) {
        const int64_t l = off[i + 1] - off[i];
        if (fr) printf("R %d\n", first + i + 1);
        if (fh) {
            const char *h = dh_dazz_header(d, i);
            printf("H %zu %s\n", strlen(h), h);
            // L <well | contig in scaffold> <begin> <end> (dazzler.d:1559-1561: length = end - begin)
            printf("L %d %d %lld\n", dh_dazz_origin(d)[i], dh_dazz_fpulse(d)[i], (long long)(dh_dazz_fpulse(d)[i] + l));
            if (!dam) printf("Q 0.%03d\n", dh_dazz_flags(d)[i] & 0x3ff);
        }
        if (fs) {
            seq.resize((size_t)l);
            for (int64_t x = 0; x < l; x++) seq[(size_t)x] = ACGT[std::min<int>(bases[off[i] + x], 4)];
            printf("S %lld %s\n", (long long)l, seq.c_str());
        }
        if (fi) {
            const int64_t a = qptr[(size_t)i], b = qptr[(size_t)i + 1];
            std::string q;
            for (int64_t x = a; x < b; x++) q.push_back(qv_char(qv[(size_t)x]));
            printf("I %lld %s\n", (long long)(b - a), q.c_str());
        }
    }
    dh_dazz_close(d);
    return 0;
}

static int tool_dbshow(const std::vector<std::string> &args)
{
    bool names = false;
    int width = 80;
    std::string db;
    std::vector<std::string> sel;
    for (const std::string &a : args) {
        if (a == "-n")
            names = true;
        else if (a.compare(0, 2, "-w") == 0)
            width = std::max(1, atoi(a.c_str() + 2));
        else if (a == "-u" || a == "-U" || a == "-q")
            ;
        else if (a[0] == '-' && !isdigit((unsigned char)a[1]))
            die("unknown option " + a);
        else if (db.empty())
            db = a;
        else
            sel.push_back(a);
    }
    if (db.empty()) die("usage: DBshow [-n] [-w<int(80)>] <path:db|dam> [ <reads:range> ... ]");
    dh_dazz *d = open_dazz(db);
    const int32_t n = dh_dazz_nreads(d), first = dh_dazz_first_id(d);
    const std::vector<int32_t> ids = record_list(sel, first, n);
    const int64_t *off = dh_dazz_offsets(d);
    const uint8_t *bases = dh_dazz_bases(d);
    const bool dam = is_dam(db) || (n > 0 && dh_dazz_header(d, 0)[0] == '>');
    static const char ACGT[] = "acgtn";
    for (int32_t i : ids) {
        const int64_t l = off[i + 1] - off[i];
        const char *h = dh_dazz_header(d, i);
        const int32_t org = dh_dazz_origin(d)[i], fp = dh_dazz_fpulse(d)[i];
        std::string head;
        if (dam) {  // `<fasta header> :: Contig <idx>[<begin>,<end>]`, dazzler.d:4689-4690
            head = std::string(h[0] == '>' ? "" : ">") + h + " :: Contig " + std::to_string(org) + "[" + std::to_string(fp) + "," +
                   std::to_string(fp + l) + "]";
        } else  // PacBio style: >prolog/well/beg_end RQ=0.xxx (dazzler.d:1389-1393)
            head = ">" + std::string(h) + "/" + std::to_string(org) + "/" + std::to_string(fp) + "_" + std::to_string(fp + l) + " RQ=0.850";
        printf("%s\n", head.c_str());
        if (names) continue;
        for (int64_t x = 0; x < l; x += width) {
            const int64_t e = std::min<int64_t>(l, x + width);
            for (int64_t y = x; y < e; y++) putchar(ACGT[std::min<int>(bases[off[i] + y], 4)]);
            putchar('\n');
        }
    }
    dh_dazz_close(d);
    return 0;
}

// ---------------------------------------------------------------------------------- device tools
struct Dev {
    dh_ctx *ctx = nullptr;
    dh_dazz *dz = nullptr;
    dh_db *db = nullptr;
};
static Dev open_dev(const std::string &path)
{
    Dev v;
    CHK(dh_ctx_create(0, nullptr, &v.ctx));
    v.dz = open_dazz(path);
    CHK(dh_db_create(v.ctx, dh_dazz_bases(v.dz), dh_dazz_offsets(v.dz), dh_dazz_nreads(v.dz), nullptr, &v.db));
    return v;
}
static void close_dev(Dev &v)
{
    dh_db_destroy(v.db);
    dh_dazz_close(v.dz);
    dh_ctx_destroy(v.ctx);
}

static int tool_dbdust(const std::vector<std::string> &args)
{
    std::string db;
    for (const std::string &a : args) {
        if (a[0] == '-') {
            if (strchr("wtmb", a[1]) == nullptr) die("unknown option " + a);
            if ((a[1] == 'w' && atoi(a.c_str() + 2) != 64) || (a[1] == 't' && fabs(atof(a.c_str() + 2) - 2.0) > 1e-9) ||
                (a[1] == 'm' && atoi(a.c_str() + 2) != 10))
                die("only the defaults -w64 -t2.0 -m10 are implemented");
        } else
            db = a;
    }
    if (db.empty()) die("usage: DBdust [-w<int(64)>] [-t<double(2.)>] [-m<int(10)>] <path:db|dam>");
    Dev v = open_dev(db);
    CHK(dh_db_dust(v.db));
    const int32_t n = dh_dazz_nreads(v.dz);
    std::vector<int64_t> ptr((size_t)n + 1);
    const int64_t m = dh_db_get_mask(v.db, ptr.data(), nullptr, 0);
    if (m < 0) die(dh_last_error());
    std::vector<int32_t> iv((size_t)std::max<int64_t>(2 * m, 2));
    dh_db_get_mask(v.db, ptr.data(), iv.data(), m);
    CHK(dh_dazz_write_mask(db.c_str(), "dust", n, ptr.data(), iv.data()));
    close_dev(v);
    return 0;
}

// overlaps of a pile-up DB: ids in the file are trimmed DB ids
static dh_la_set *read_las(const std::string &path, std::vector<dh_la> &las, int32_t first)
{
    dh_la_set *set = nullptr;
    CHK(dh_las_read(path.c_str(), &set));
    const int64_t n = dh_la_set_count(set);
    las.assign(dh_la_set_records(set), dh_la_set_records(set) + n);
    for (dh_la &l : las) {
        l.aread -= first;
        l.bread -= first;
    }
    return set;
}

// DAScover + DASqv / computeintrinsicqv: intrinsic QV per trace tile of every read -> byte track
static int tool_qv(const char *track, const std::vector<std::string> &args, bool write)
{
    int cov = 0;
    std::vector<std::string> pos;
    for (const std::string &a : args) {
        if (a == "-v")
            ;
        else if (a.compare(0, 2, "-c") == 0 || a.compare(0, 2, "-d") == 0)
            cov = atoi(a.c_str() + 2);
        else if (a.compare(0, 2, "-m") == 0 || a.compare(0, 2, "-H") == 0)
            ;
        else if (a[0] == '-')
            die("unknown option " + a);
        else
            pos.push_back(a);
    }
    if (pos.size() != 2) die(std::string("usage: ") + g_tool + " [-v] [-c<int>|-d<int>] <db> <las>");
    if (!write) return 0;  // DAScover: the coverage estimate is folded into DASqv's -c here
    Dev v = open_dev(pos[0]);
    std::vector<dh_la> las;
    dh_la_set *set = read_las(pos[1], las, dh_dazz_first_id(v.dz));
    const int32_t n = dh_dazz_nreads(v.dz), ts = dh_la_set_tspace(set);
    if (cov <= 0) cov = std::max(4, n);
    const int64_t *off = dh_dazz_offsets(v.dz);
    int32_t maxtiles = 1;
    for (int32_t i = 0; i < n; i++) maxtiles = std::max<int32_t>(maxtiles, (int32_t)((off[i + 1] - off[i] + ts - 1) / ts));
    std::vector<uint8_t> qv((size_t)n * maxtiles, 255);
    CHK(dh_tile_qv(v.ctx, v.db, las.data(), (int64_t)las.size(), dh_la_set_trace(set), ts, cov, qv.data(), maxtiles));
    std::vector<int64_t> ptr((size_t)n + 1, 0);
    std::vector<uint8_t> data;
    for (int32_t i = 0; i < n; i++) {
        const int32_t nt = (int32_t)((off[i + 1] - off[i] + ts - 1) / ts);
        for (int32_t t = 0; t < nt; t++) data.push_back(std::min<uint8_t>(qv[(size_t)i * maxtiles + t], 50));
        ptr[(size_t)i + 1] = (int64_t)data.size();
    }
    data.push_back(0);
    CHK(dh_dazz_write_track(pos[0].c_str(), track, n, ptr.data(), data.data()));
    dh_la_set_destroy(set);
    close_dev(v);
    return 0;
}

static int tool_daccord(const std::vector<std::string> &args)
{
    int i0 = -1, i1 = -1, rounds = 3;
    bool eprof_only = false;
    std::vector<std::string> pos;
    for (const std::string &a : args) {
        if (a.compare(0, 2, "-I") == 0) {
            if (sscanf(a.c_str() + 2, "%d,%d", &i0, &i1) != 2) die("bad -I");
        } else if (a == "--eprofonly")
            eprof_only = true;
        else if (a == "-f" || a.compare(0, 2, "-t") == 0 || a.compare(0, 2, "-w") == 0 || a.compare(0, 2, "-a") == 0 ||
                 a.compare(0, 2, "-k") == 0 || a.compare(0, 2, "-m") == 0 || a.compare(0, 2, "-d") == 0 || a.compare(0, 2, "-V") == 0)
            ;
        else if (a.compare(0, 9, "--rounds=") == 0)
            rounds = atoi(a.c_str() + 9);
        else if (a[0] == '-')
            die("unknown option " + a);
        else
            pos.push_back(a);
    }
    if (pos.size() != 2) die("usage: daccord [-t<n>] [-I<i>,<j>] [-f] [--eprofonly] <las> <db>");
    if (eprof_only) {  // the error profile pass: this consensus needs none, the file marks it as done
        FILE *f = fopen((pos[0] + ".eprof").c_str(), "wb");
        if (!f) die("cannot write " + pos[0] + ".eprof");
        fputs("dentist-hip: no error profile needed\n", f);
        fclose(f);
        return 0;
    }
    Dev v = open_dev(pos[1]);
    std::vector<dh_la> las;
    dh_la_set *set = read_las(pos[0], las, dh_dazz_first_id(v.dz));
    const int32_t n = dh_dazz_nreads(v.dz), ts = dh_la_set_tspace(set);
    if (i0 < 0) {
        i0 = 0;
        i1 = n - 1;
    }
    if (i0 > i1 || i1 >= n) die("-I outside the DB");
    const int64_t *off = dh_dazz_offsets(v.dz);
    static const char ACGT[] = "acgtn";
    for (int32_t r = i0; r <= i1; r++) {
        std::vector<uint8_t> out((size_t)(off[r + 1] - off[r]) * 6 + 64);
        int64_t len = 0;
        CHK(dh_consensus(v.ctx, v.db, las.data(), (int64_t)las.size(), dh_la_set_trace(set), ts, r, rounds, out.data(),
                         (int64_t)out.size(), &len));
        // header in daccord's style: read id (0-based) / segment / 0_length
        printf(">%d/0/0_%lld A=[0,%lld]\n", r, (long long)len, (long long)len);
        for (int64_t x = 0; x < len; x += 80) {
            for (int64_t y = x; y < std::min(len, x + 80); y++) putchar(ACGT[std::min<int>(out[(size_t)y], 4)]);
            putchar('\n');
        }
    }
    dh_la_set_destroy(set);
    close_dev(v);
    return 0;
}

static int tool_lamerge(const std::vector<std::string> &args)
{
    std::vector<const char *> in;
    std::string out;
    for (const std::string &a : args) {
        if (a == "-v" || a == "-a" || a.compare(0, 2, "-P") == 0)
            continue;
        if (a[0] == '-') die("unknown option " + a);
        if (out.empty())
            out = a;
        else
            in.push_back(a.c_str());
    }
    if (out.empty() || in.empty()) die("usage: LAmerge [-va] <merge:las> <parts:las> ...");
    if (out.size() < 4 || out.compare(out.size() - 4, 4, ".las") != 0) out += ".las";
    CHK(dh_las_merge(in.data(), (int32_t)in.size(), out.c_str()));
    return 0;
}

// ---------------------------------------------------------------------------------- workflow helpers (host only)
// LAsplit: the records of a .las on stdin in <parts> files of nearly equal size; a file ends only where the A read changes
// (the piles of an A read stay together: every consumer of a block file reads piles).  '@' or '#' in the target is the
// part number, 1-based.
static int tool_lasplit(const std::vector<std::string> &args)
{
    std::vector<std::string> pos;
    for (const std::string &a : args) {
        if (a == "-v") continue;
        if (a[0] == '-' && a.size() > 1) die("unknown option " + a);
        pos.push_back(a);
    }
    if (pos.size() != 2) die("usage: LAsplit <target:path with @> <parts:int> < <source>.las");
    const int32_t parts = atoi(pos[1].c_str());
    const size_t mark = pos[0].find_first_of("@#");
    if (parts < 1 || mark == std::string::npos) die("LAsplit: the target needs a '@' (or '#') and parts >= 1 (a DB as the second argument is not supported)");
    // the codec works on files: stdin goes through a temporary one next to the first target
    std::string tmp = pos[0];
    tmp.replace(mark, 1, "stdin-tmp");
    if (tmp.size() < 4 || tmp.compare(tmp.size() - 4, 4, ".las") != 0) tmp += ".las";
    {
        const std::string raw = slurp(stdin);
        FILE *f = fopen(tmp.c_str(), "wb");
        if (!f || fwrite(raw.data(), 1, raw.size(), f) != raw.size() || fclose(f) != 0) die("cannot write " + tmp);
    }
    dh_la_set *set = nullptr;
    const int rc = dh_las_read(tmp.c_str(), &set);
    remove(tmp.c_str());
    if (rc) die(std::string("dh_las_read: ") + dh_last_error());
    const int64_t n = dh_la_set_count(set);
    const dh_la *la = dh_la_set_records(set);
    const uint16_t *tr = dh_la_set_trace(set);
    const int32_t ts = dh_la_set_tspace(set);
    int64_t at = 0;
    for (int32_t k = 1; k <= parts; k++) {
        int64_t end = k == parts ? n : std::min<int64_t>(n, (n * k + parts - 1) / parts);
        end = std::max(end, at);
        while (end > at && end < n && la[end].aread == la[end - 1].aread) end++;  // do not cut a pile
        std::string out = pos[0];
        out.replace(mark, 1, std::to_string(k));
        if (out.size() < 4 || out.compare(out.size() - 4, 4, ".las") != 0) out += ".las";
        // (records keep their trace offsets into the whole trace array)
        CHK(dh_las_write(out.c_str(), la + at, end - at, tr, ts));
        at = end;
    }
    dh_la_set_destroy(set);
    return 0;
}

struct DbPath {
    std::string dir, root, ext;  // dir/root.ext (ext "db" or "dam"), block > 0 when the path names one
    int32_t block = 0;
};
static DbPath parse_db_path(std::string p)
{
    DbPath d;
    const size_t sl = p.find_last_of('/');
    d.dir = sl == std::string::npos ? "." : p.substr(0, sl);
    std::string base = sl == std::string::npos ? p : p.substr(sl + 1);
    for (const char *e : {".dam", ".db"})
        if (base.size() > strlen(e) && base.compare(base.size() - strlen(e), strlen(e), e) == 0) base.resize(base.size() - strlen(e));
    const size_t dot = base.find_last_of('.');
    if (dot != std::string::npos && dot + 1 < base.size() && base.find_first_not_of("0123456789", dot + 1) == std::string::npos) {
        d.block = atoi(base.c_str() + dot + 1);
        base.resize(dot);
    }
    d.root = base;
    for (const char *e : {"dam", "db"}) {
        FILE *f = fopen((d.dir + "/" + d.root + "." + e).c_str(), "r");
        if (f) {
            fclose(f);
            d.ext = e;
            break;
        }
    }
    if (d.ext.empty()) die("DAZZ_DB not found: " + p);
    return d;
}
static int32_t stub_blocks(const DbPath &d)
{
    FILE *f = fopen((d.dir + "/" + d.root + "." + d.ext).c_str(), "r");
    if (!f) die("cannot open the DB stub");
    char line[512];
    int32_t nb = 0;
    while (fgets(line, sizeof(line), f))
        if (sscanf(line, "blocks = %d", &nb) == 1) break;
    fclose(f);
    return nb;
}
static std::string track_file(const DbPath &d, int32_t block, const std::string &name, const char *ext)
{
    return d.dir + "/." + d.root + (block > 0 ? "." + std::to_string(block) : "") + "." + name + "." + ext;
}
static void write_mask_files(const DbPath &d, int32_t block, const std::string &name, int32_t nreads, const std::vector<int64_t> &ptr,
                             const std::vector<int32_t> &iv)
{
    FILE *an = fopen(track_file(d, block, name, "anno").c_str(), "wb"), *da = fopen(track_file(d, block, name, "data").c_str(), "wb");
    if (!an || !da) die("cannot create the track files of " + name);
    const int32_t head[2] = {nreads, 0};  // size 0 marks a mask track (dazzler.d:5143)
    bool ok = fwrite(head, 4, 2, an) == 2;
    for (int32_t i = 0; i <= nreads; i++) {
        const int64_t off = ptr[(size_t)i] * 2 * (int64_t)sizeof(int32_t);
        ok = ok && fwrite(&off, 8, 1, an) == 1;
    }
    if (!iv.empty()) ok = ok && fwrite(iv.data(), 4, iv.size(), da) == iv.size();
    ok = (fclose(an) == 0) && ok;
    ok = (fclose(da) == 0) && ok;
    if (!ok) die("short write of the track files of " + name);
}

// Catrack: the block tracks of a mask concatenated into the track of the whole DB
static int tool_catrack(const std::vector<std::string> &args)
{
    std::vector<std::string> pos;
    bool del = false;
    for (const std::string &a : args) {
        if (a == "-v" || a == "-f") continue;
        if (a == "-d") {
            del = true;
            continue;
        }
        if (a[0] == '-') die("unknown option " + a);
        pos.push_back(a);
    }
    if (pos.size() != 2) die("usage: Catrack [-vfd] <path:db|dam> <track:name>");
    const DbPath d = parse_db_path(pos[0]);
    const int32_t nb = stub_blocks(d);
    if (nb < 1) die("Catrack: the DB has not been split (DBsplit)");
    std::vector<int64_t> ptr{0};
    std::vector<int32_t> iv;
    int32_t nreads = 0;
    for (int32_t b = 1; b <= nb; b++) {
        FILE *an = fopen(track_file(d, b, pos[1], "anno").c_str(), "rb"), *da = fopen(track_file(d, b, pos[1], "data").c_str(), "rb");
        if (!an || !da) die("Catrack: track " + pos[1] + " of block " + std::to_string(b) + " is missing");
        int32_t head[2];
        if (fread(head, 4, 2, an) != 2 || head[1] != 0 || head[0] < 0) die("Catrack: not a mask track (block " + std::to_string(b) + ")");
        std::vector<int64_t> offs((size_t)head[0] + 1);
        if (fread(offs.data(), 8, offs.size(), an) != offs.size()) die("Catrack: truncated .anno of block " + std::to_string(b));
        fclose(an);
        std::vector<int32_t> data;
        int32_t buf[4096];
        size_t got;
        while ((got = fread(buf, 4, 4096, da)) > 0) data.insert(data.end(), buf, buf + got);
        fclose(da);
        if (offs[0] != 0 || offs.back() != (int64_t)data.size() * 4) die("Catrack: .anno and .data of block " + std::to_string(b) + " disagree");
        const int64_t base = ptr.back();
        for (int32_t i = 1; i <= head[0]; i++) {
            if (offs[(size_t)i] < offs[(size_t)i - 1] || offs[(size_t)i] % 8) die("Catrack: corrupted offsets");
            ptr.push_back(base + offs[(size_t)i] / 8);
        }
        iv.insert(iv.end(), data.begin(), data.end());
        nreads += head[0];
    }
    write_mask_files(d, 0, pos[1], nreads, ptr, iv);
    if (del)
        for (int32_t b = 1; b <= nb; b++) {
            remove(track_file(d, b, pos[1], "anno").c_str());
            remove(track_file(d, b, pos[1], "data").c_str());
        }
    return 0;
}

// TANmask: a local alignment of a read with itself (datander) marks a tandem repeat -- the union of its A and B intervals,
// when at least -l long, goes into the mask; intervals of a read are merged.  One track per .las: the block's when the
// file name carries a block number (TAN.<db>.<block>.las), the DB's otherwise.
static int tool_tanmask(const std::vector<std::string> &args)
{
    std::vector<std::string> pos;
    int32_t minlen = 500;
    std::string name = "tan";
    for (const std::string &a : args) {
        if (a == "-v") continue;
        if (a.compare(0, 2, "-l") == 0 && a.size() > 2)
            minlen = atoi(a.c_str() + 2);
        else if (a.compare(0, 2, "-n") == 0 && a.size() > 2)
            name = a.substr(2);
        else if (a[0] == '-')
            die("unknown option " + a);
        else
            pos.push_back(a);
    }
    if (pos.size() < 2) die("usage: TANmask [-v] [-l<int(500)>] [-n<track(tan)>] <subject:db|dam> <overlaps:las> ...");
    const DbPath d = parse_db_path(pos[0]);
    for (size_t f = 1; f < pos.size(); f++) {
        std::string lp = pos[f];
        if (lp.size() < 4 || lp.compare(lp.size() - 4, 4, ".las") != 0) lp += ".las";
        // block of the file: "<...>.<root>.<block>.las"
        int32_t block = 0;
        {
            const std::string stem = lp.substr(0, lp.size() - 4);
            const size_t dot = stem.find_last_of('.');
            if (dot != std::string::npos && dot + 1 < stem.size() && stem.find_first_not_of("0123456789", dot + 1) == std::string::npos)
                block = atoi(stem.c_str() + dot + 1);
        }
        dh_dazz *db = open_dazz(d.dir + "/" + d.root + (block > 0 ? "." + std::to_string(block) : "") + "." + d.ext);
        const int32_t n = dh_dazz_nreads(db), first = dh_dazz_first_id(db);
        dh_la_set *set = nullptr;
        CHK(dh_las_read(lp.c_str(), &set));
        const int64_t nl = dh_la_set_count(set);
        const dh_la *la = dh_la_set_records(set);
        std::vector<std::vector<std::pair<int32_t, int32_t>>> per((size_t)n);
        for (int64_t i = 0; i < nl; i++) {
            if (la[i].aread != la[i].bread || (la[i].flags & DH_FLAG_COMP)) continue;
            const int32_t r = la[i].aread - first;
            if (r < 0 || r >= n) die("TANmask: read id outside the DB block");
            const int32_t b = std::min(la[i].abpos, la[i].bbpos), e = std::max(la[i].aepos, la[i].bepos);
            if (e - b >= minlen) per[(size_t)r].emplace_back(b, e);
        }
        std::vector<int64_t> ptr{0};
        std::vector<int32_t> iv;
        for (int32_t r = 0; r < n; r++) {
            auto &v = per[(size_t)r];
            std::sort(v.begin(), v.end());
            size_t at = iv.size();
            for (const auto &x : v) {
                if (iv.size() > at && x.first <= iv.back())
                    iv.back() = std::max(iv.back(), x.second);
                else {
                    iv.push_back(x.first);
                    iv.push_back(x.second);
                }
            }
            ptr.push_back((int64_t)iv.size() / 2);
        }
        write_mask_files(d, block, name, n, ptr, iv);
        dh_la_set_destroy(set);
        dh_dazz_close(db);
    }
    return 0;
}

static int tool_merge_insertions(const std::vector<std::string> &args)
{
    std::vector<const char *> in;
    std::string out;
    for (const std::string &a : args) {
        if (a == "-v" || a == "-vv" || a == "-vvv") continue;
        if (a[0] == '-') die("unknown option " + a);
        if (out.empty())
            out = a;
        else
            in.push_back(a.c_str());
    }
    if (out.empty() || in.empty()) die("usage: merge-insertions <merged-insertions:db> <insertions:db> ...");
    int64_t n = 0;
    CHK(dh_insertiondb_merge(in.data(), (int32_t)in.size(), out.c_str(), &n));
    fprintf(stderr, "{\"numInputFiles\":%zu,\"totalNumInsertions\":%lld}\n", in.size(), (long long)n);
    return 0;
}

// ---------------------------------------------------------------------------------- LApaf
// One PAF line per record: the query is the B read (strand '-' and coordinates turned back to the forward strand for
// complement records), the target the A sequence; names are the first word of the FASTA header (DAM) or the prolog (DB)
// followed by /<1-based read number>.  Tags: NM:i the exact edit distance summed over the trace tiles, tp:i the sum of the
// trace's diffs (what the aligner's band found), cg:Z the extended cigar (= X I D).
// -c: one line per CHAIN of the file (a record without the NEXT flag starts a chain, file order), from dh_la_chain_paths: the
// query range is the chain's B range, the target range its A range; NM:i the non-zero ops, nl:i the records of the chain, nf:i
// the fillers aligned between them, cg:Z the cigar of the whole chain; fk:i:1 on a chain with a faked filler; a nested chain
// prints 0 matches, * for the cigar and st:Z:nested.  first-last counts chains then.
static std::string paf_name(const dh_dazz *d, int32_t i)
{
    const char *h = dh_dazz_header(d, i);
    std::string s = h ? h : "";
    if (!s.empty() && s[0] == '>') s.erase(0, 1);
    const size_t e = s.find_first_of(" \t\n");
    if (e != std::string::npos) s.resize(e);
    if (s.empty()) s = "read";
    return s + "/" + std::to_string(dh_dazz_first_id(d) + i + 1);
}

static int tool_lapaf(const std::vector<std::string> &args)
{
    bool show = false, chains = false;
    int width = 100;
    std::vector<std::string> pos;
    for (const std::string &a : args) {
        if (a == "-a")
            show = true;
        else if (a == "-c")
            chains = true;
        else if (a.compare(0, 2, "-w") == 0)
            width = atoi(a.c_str() + 2);
        else if (a[0] == '-')
            die("unknown option " + a);
        else
            pos.push_back(a);
    }
    long long r0 = 1, r1 = -1;
    if (pos.size() >= 3 && pos.back().find_first_not_of("0123456789-") == std::string::npos) {
        if (sscanf(pos.back().c_str(), "%lld-%lld", &r0, &r1) != 2) {
            if (sscanf(pos.back().c_str(), "%lld", &r0) != 1) die("bad record range " + pos.back());
            r1 = r0;
        }
        pos.pop_back();
    }
    if (pos.size() < 2 || pos.size() > 3 || width < 1) die("usage: LApaf [-a] [-c] [-w<int(100)>] <A:db|dam> [<B:db|dam>] <align:las> [first-last]");
    const bool two = pos.size() == 3 && pos[1] != pos[0];
    Dev va = open_dev(pos[0]);
    Dev vb;
    if (two) {
        vb.dz = open_dazz(pos[1]);
        CHK(dh_db_create(va.ctx, dh_dazz_bases(vb.dz), dh_dazz_offsets(vb.dz), dh_dazz_nreads(vb.dz), nullptr, &vb.db));
    }
    const dh_dazz *da = va.dz, *dbz = two ? vb.dz : va.dz;
    dh_db *A = va.db, *B = two ? vb.db : va.db;
    dh_la_set *set = nullptr;
    CHK(dh_las_read(pos.back().c_str(), &set));
    const int64_t n = dh_la_set_count(set);
    std::vector<dh_la> las(dh_la_set_records(set), dh_la_set_records(set) + n);
    for (dh_la &l : las) {
        l.aread -= dh_dazz_first_id(da);
        l.bread -= dh_dazz_first_id(dbz);
    }
    // the entries of the output: records, or (-c) chains by flags as record ranges
    std::vector<int64_t> coff;
    if (chains) {
        for (int64_t i = 0; i < n; i++)
            if (i == 0 || !(las[(size_t)i].flags & DH_FLAG_NEXT)) coff.push_back(i);
        coff.push_back(n);
    }
    const int64_t nent = chains ? (int64_t)coff.size() - 1 : n;
    if (r1 < 0) r1 = nent;
    if (r0 < 1 || r1 > nent || r0 > r1 + 1)
        die(std::string(chains ? "chain" : "record") + " range outside the file (" + std::to_string(nent) + (chains ? " chains)" : " records)"));
    const uint16_t *trace = dh_la_set_trace(set);
    const int32_t ts = dh_la_set_tspace(set);
    dh_edit_paths *ep = nullptr;
    std::vector<int32_t> cstatus;
    if (chains) {
        const int64_t cnt = r1 - r0 + 1, rec0 = coff[(size_t)(r0 - 1)];
        std::vector<int64_t> off((size_t)cnt + 1);
        for (int64_t k = 0; k <= cnt; k++) off[(size_t)k] = coff[(size_t)(r0 - 1 + k)] - rec0;
        cstatus.assign((size_t)cnt + 1, 0);
        CHK(dh_la_chain_paths(va.ctx, A, B, las.data() + rec0, n - rec0, trace, ts, off.data(), cnt, &ep, cstatus.data()));
    } else {
        CHK(dh_la_edit_paths(va.ctx, A, B, las.data(), n, trace, ts, r0 - 1, r1 - r0 + 1, &ep));
    }
    const int64_t *op_off = dh_edit_paths_op_off(ep);
    const uint8_t *ops = dh_edit_paths_ops(ep);
    const int32_t *score = dh_edit_paths_score(ep);
    const int32_t *nfill = dh_edit_paths_entry_fillers(ep);
    const int64_t *aoff = dh_dazz_offsets(da), *boff = dh_dazz_offsets(dbz);
    std::vector<char> text;
    std::vector<uint8_t> brc;
    for (int64_t i = 0; i < dh_edit_paths_count(ep); i++) {
        // the entry as one record: a chain from the begin of its first record to the end of its last
        const int64_t f = chains ? coff[(size_t)(r0 - 1 + i)] : r0 - 1 + i, e = chains ? coff[(size_t)(r0 + i)] : f + 1;
        dh_la l = las[(size_t)f];
        l.aepos = las[(size_t)(e - 1)].aepos;
        l.bepos = las[(size_t)(e - 1)].bepos;
        const uint8_t *o = ops + op_off[i];
        const int64_t no = op_off[i + 1] - op_off[i];
        const int64_t alen = aoff[l.aread + 1] - aoff[l.aread], blen = boff[l.bread + 1] - boff[l.bread];
        const bool comp = (l.flags & DH_FLAG_COMP) != 0;
        const bool nested = chains && cstatus[(size_t)i] == DH_CP_NESTED;
        int64_t nmatch = 0, tdiffs = 0;
        for (int64_t k = 0; k < no; k++) nmatch += o[k] == 0;
        for (int32_t t = 0; t < l.tlen; t += 2) tdiffs += trace[l.toff + t];
        const int64_t clen = dh_format_cigar(o, no, 1, nullptr, 0);
        if (clen < 0) die(dh_last_error());
        text.resize((size_t)clen + 1);
        dh_format_cigar(o, no, 1, text.data(), clen + 1);
        printf("%s\t%lld\t%lld\t%lld\t%c\t%s\t%lld\t%d\t%d\t%lld\t%lld\t255\tNM:i:%d", paf_name(dbz, l.bread).c_str(), (long long)blen,
               (long long)(comp ? blen - l.bepos : l.bbpos), (long long)(comp ? blen - l.bbpos : l.bepos), comp ? '-' : '+',
               paf_name(da, l.aread).c_str(), (long long)alen, l.abpos, l.aepos, (long long)nmatch, (long long)no, score[i]);
        if (!chains) {
            printf("\ttp:i:%lld\tcg:Z:%s\n", (long long)tdiffs, text.data());
        } else {
            printf("\tnl:i:%lld\tnf:i:%d\tcg:Z:%s", (long long)(e - f), nfill ? nfill[i] : 0, nested ? "*" : text.data());
            if (cstatus[(size_t)i] == DH_CP_FAKED) printf("\tfk:i:1");
            if (nested) printf("\tst:Z:nested");
            putchar('\n');
        }
        if (!show || nested) continue;
        const uint8_t *a = dh_dazz_bases(da) + aoff[l.aread] + l.abpos, *b = dh_dazz_bases(dbz) + boff[l.bread] + l.bbpos;
        if (comp) {  // the B side of the record in the reverse-complement frame
            brc.resize((size_t)(l.bepos - l.bbpos));
            const uint8_t *fwd = dh_dazz_bases(dbz) + boff[l.bread];
            for (int32_t x = l.bbpos; x < l.bepos; x++) {
                const uint8_t c = fwd[blen - 1 - x];
                brc[(size_t)(x - l.bbpos)] = c < 4 ? (uint8_t)(3 - c) : c;
            }
            b = brc.data();
        }
        const int64_t tl = dh_format_alignment(a, b, o, no, width, nullptr, 0);
        if (tl < 0) die(dh_last_error());
        text.resize((size_t)tl + 1);
        dh_format_alignment(a, b, o, no, width, text.data(), tl + 1);
        putchar('#');
        for (int64_t k = 0; k < tl; k++) {
            putchar(text[(size_t)k]);
            if (text[(size_t)k] == '\n') putchar('#');
        }
        putchar('\n');
    }
    dh_edit_paths_destroy(ep);
    dh_la_set_destroy(set);
    if (two) {
        dh_db_destroy(vb.db);
        dh_dazz_close(vb.dz);
    }
    close_dev(va);
    return 0;
}

// ---------------------------------------------------------------------------------- LAtranspose
static int tool_latranspose(const std::vector<std::string> &args)
{
    bool best = false;
    std::vector<std::string> pos;
    for (const std::string &a : args) {
        if (a == "-b")
            best = true;
        else if (a[0] == '-')
            die("unknown option " + a);
        else
            pos.push_back(a);
    }
    if (pos.size() != 4) die("usage: LAtranspose [-b] <A:db|dam> <B:db|dam> <in:las> <out:las>");
    const bool two = pos[1] != pos[0];
    Dev va = open_dev(pos[0]);
    Dev vb;
    if (two) {
        vb.dz = open_dazz(pos[1]);
        CHK(dh_db_create(va.ctx, dh_dazz_bases(vb.dz), dh_dazz_offsets(vb.dz), dh_dazz_nreads(vb.dz), nullptr, &vb.db));
    }
    const dh_dazz *da = va.dz, *dbz = two ? vb.dz : va.dz;
    dh_db *A = va.db, *B = two ? vb.db : va.db;
    dh_la_set *set = nullptr, *out = nullptr;
    CHK(dh_las_read(pos[2].c_str(), &set));
    const int64_t n = dh_la_set_count(set);
    std::vector<dh_la> las(dh_la_set_records(set), dh_la_set_records(set) + n);
    for (dh_la &l : las) {
        l.aread -= dh_dazz_first_id(da);
        l.bread -= dh_dazz_first_id(dbz);
    }
    CHK(dh_la_transpose(va.ctx, A, B, las.data(), n, dh_la_set_trace(set), dh_la_set_tspace(set), best ? 1 : 0, &out, nullptr));
    las.assign(dh_la_set_records(out), dh_la_set_records(out) + dh_la_set_count(out));
    for (dh_la &l : las) {  // (the id offsets exchanged with the reads)
        l.aread += dh_dazz_first_id(dbz);
        l.bread += dh_dazz_first_id(da);
    }
    CHK(dh_las_write(pos[3].c_str(), las.data(), (int64_t)las.size(), dh_la_set_trace(out), dh_la_set_tspace(out)));
    dh_la_set_destroy(out);
    dh_la_set_destroy(set);
    if (two) {
        dh_db_destroy(vb.db);
        dh_dazz_close(vb.dz);
    }
    close_dev(va);
    return 0;
}

// ---------------------------------------------------------------------------------- DBnw
// Read i of A against read i of B, globally (dh_nw_batch; -f: free shift).  One line per pair, tab separated: pair number
// (1-based), length of the A read, length of the B read, score, matches, alignment columns (the two numbers
// `check-results` reads from stretcher's "# Identity:" line), extended cigar.  A pair whose band the kernel does not serve
// prints score -1, 0 matches, 0 columns and the cigar "*".
static int tool_dbnw(const std::vector<std::string> &args)
{
    bool show = false, fs = false;
    int width = 100;
    std::vector<std::string> pos;
    for (const std::string &a : args) {
        if (a == "-a")
            show = true;
        else if (a == "-f")
            fs = true;
        else if (a.compare(0, 2, "-w") == 0)
            width = atoi(a.c_str() + 2);
        else if (a[0] == '-')
            die("unknown option " + a);
        else
            pos.push_back(a);
    }
    long long r0 = 1, r1 = -1;
    if (pos.size() >= 3 && pos.back().find_first_not_of("0123456789-") == std::string::npos) {
        if (sscanf(pos.back().c_str(), "%lld-%lld", &r0, &r1) != 2) {
            if (sscanf(pos.back().c_str(), "%lld", &r0) != 1) die("bad pair range " + pos.back());
            r1 = r0;
        }
        pos.pop_back();
    }
    if (pos.size() != 2 || width < 1) die("usage: DBnw [-f] [-a] [-w<int(100)>] <A:db|dam> <B:db|dam> [first-last]");
    dh_ctx *ctx = nullptr;
    CHK(dh_ctx_create(0, nullptr, &ctx));
    dh_dazz *da = open_dazz(pos[0]), *dbz = open_dazz(pos[1]);
    const int64_t n = std::min(dh_dazz_nreads(da), dh_dazz_nreads(dbz));
    if (r1 < 0) r1 = n;
    if (r0 < 1 || r1 > n || r0 > r1 + 1) die("pair range outside the DBs (" + std::to_string(n) + " pairs)");
    const int64_t cnt = r1 - r0 + 1;
    const int64_t *aoff = dh_dazz_offsets(da) + (r0 - 1), *boff = dh_dazz_offsets(dbz) + (r0 - 1);
    dh_edit_paths *ep = nullptr;
    std::vector<int32_t> status((size_t)cnt + 1);
    CHK(dh_nw_batch(ctx, dh_dazz_bases(da), aoff, dh_dazz_bases(dbz), boff, cnt, fs ? 1 : 0, &ep, status.data()));
    const int64_t *op_off = dh_edit_paths_op_off(ep);
    const uint8_t *ops = dh_edit_paths_ops(ep);
    const int32_t *score = dh_edit_paths_score(ep);
    std::vector<char> text;
    for (int64_t i = 0; i < cnt; i++) {
        const uint8_t *o = ops + op_off[i];
        const int64_t no = op_off[i + 1] - op_off[i];
        const long long alen = aoff[i + 1] - aoff[i], blen = boff[i + 1] - boff[i];
        if (status[(size_t)i] != DH_NW_OK) {
            printf("%lld\t%lld\t%lld\t-1\t0\t0\t*\n", (long long)(r0 + i), alen, blen);
            continue;
        }
        int64_t nmatch = 0;
        for (int64_t k = 0; k < no; k++) nmatch += o[k] == 0;
        const int64_t clen = dh_format_cigar(o, no, 1, nullptr, 0);
        if (clen < 0) die(dh_last_error());
        text.resize((size_t)clen + 1);
        text[0] = 0;
        dh_format_cigar(o, no, 1, text.data(), clen + 1);
        printf("%lld\t%lld\t%lld\t%d\t%lld\t%lld\t%s\n", (long long)(r0 + i), alen, blen, score[i], (long long)nmatch, (long long)no,
               text.data());
        if (!show) continue;
        const int64_t tl = dh_format_alignment(dh_dazz_bases(da) + aoff[i], dh_dazz_bases(dbz) + boff[i], o, no, width, nullptr, 0);
        if (tl < 0) die(dh_last_error());
        text.resize((size_t)tl + 1);
        text[0] = 0;
        dh_format_alignment(dh_dazz_bases(da) + aoff[i], dh_dazz_bases(dbz) + boff[i], o, no, width, text.data(), tl + 1);
        putchar('#');
        for (int64_t k = 0; k < tl; k++) {
            putchar(text[(size_t)k]);
            if (text[(size_t)k] == '\n') putchar('#');
        }
        putchar('\n');
    }
    dh_edit_paths_destroy(ep);
    dh_dazz_close(dbz);
    dh_dazz_close(da);
    dh_ctx_destroy(ctx);
    return 0;
}

// ---------------------------------------------------------------------------------- stretcher
// The first record of a FASTA file: its name (the header's first word) and its bases as codes 0..4 (letters outside ACGT
// become N).
static void first_fasta_record(const std::string &path, std::string &name, std::vector<uint8_t> &seq)
{
    FILE *f = fopen(path.c_str(), "r");
    if (!f) die("cannot open " + path);
    const std::string text = slurp(f);
    fclose(f);
    size_t p = text.find('>');
    if (p == std::string::npos || (p > 0 && text[p - 1] != '\n')) die("no FASTA record in " + path);
    size_t eol = text.find('\n', p);
    if (eol == std::string::npos) eol = text.size();
    const std::string header = text.substr(p + 1, eol - p - 1);
    name = header.substr(0, header.find_first_of(" \t\r"));
    for (size_t k = eol; k < text.size(); k++) {
        const char c = text[k];
        if (c == '>' && text[k - 1] == '\n') break;
        if (c == '\n' || c == '\r' || c == ' ' || c == '\t') continue;
        switch (c | 32) {
            case 'a': seq.push_back(0); break;
            case 'c': seq.push_back(1); break;
            case 'g': seq.push_back(2); break;
            case 't': seq.push_back(3); break;
            default: seq.push_back(4);
        }
    }
}

static int tool_stretcher(const std::vector<std::string> &args)
{
    const char *usage = "usage: stretcher [--auto] [--stdout | --outfile=<file>] [--aformat=pair] [--awidth=<int(50)>] [--sreverse2] "
                        "[--gapopen=<int(16)>] [--gapextend=<int(4)>] <a:fasta> <b:fasta>";
    dh_nw_scoring sc = {5, -4, 16, 4};
    long long width = 50;
    bool rev2 = false;
    std::string outfile;
    std::vector<std::string> pos;
    for (const std::string &a : args) {
        if (a.size() < 2 || a[0] != '-') {
            pos.push_back(a);
            continue;
        }
        const std::string opt = a.substr(a[1] == '-' ? 2 : 1);
        const size_t eq = opt.find('=');
        const std::string key = opt.substr(0, eq), val = eq == std::string::npos ? "" : opt.substr(eq + 1);
        char *end = nullptr;
        const long long num = strtoll(val.c_str(), &end, 10);
        const bool is_num = !val.empty() && *end == 0;
        if ((key == "auto" || key == "stdout") && eq == std::string::npos)
            ;
        else if (key == "sreverse2" && eq == std::string::npos)
            rev2 = true;
        else if (key == "aformat") {
            if (val != "pair") die("--aformat=" + val + ": only the pair format is written");
        } else if (key == "awidth" && is_num && num >= 1)
            width = num;
        else if (key == "gapopen" && is_num && num >= 0 && num <= INT32_MAX)
            sc.gap_open = (int32_t)num;
        else if (key == "gapextend" && is_num && num >= 0 && num <= INT32_MAX)
            sc.gap_extend = (int32_t)num;
        else if (key == "outfile" && !val.empty())
            outfile = val;
        else
            die("unknown or malformed option " + a + "\n" + usage);
    }
    if (pos.size() != 2) die(usage);
    std::string name[2];
    std::vector<uint8_t> seq[2];
    for (int k = 0; k < 2; k++) first_fasta_record(pos[(size_t)k], name[k], seq[k]);
    if (rev2) {
        std::reverse(seq[1].begin(), seq[1].end());
        for (uint8_t &c : seq[1]) c = c < 4 ? (uint8_t)(3 - c) : c;
    }
    dh_ctx *ctx = nullptr;
    CHK(dh_ctx_create(0, nullptr, &ctx));
    const int64_t aoff[2] = {0, (int64_t)seq[0].size()}, boff[2] = {0, (int64_t)seq[1].size()};
    dh_edit_paths *ep = nullptr;
    int32_t status = 0;
    CHK(dh_nw_affine_batch(ctx, seq[0].data(), aoff, seq[1].data(), boff, 1, &sc, &ep, &status));
    if (status != DH_NW_OK)
        die("the alignment of " + name[0] + " (" + std::to_string(seq[0].size()) + " bases) and " + name[1] + " (" +
                std::to_string(seq[1].size()) + " bases) cannot be proven optimal inside " + std::to_string(DH_NWA_MAX_BAND) +
                " diagonals, the widest band the kernel serves; nothing was written",
            2);
    const uint8_t *ops = dh_edit_paths_ops(ep);
    const int64_t nops = dh_edit_paths_op_off(ep)[1];
    const int32_t score = dh_edit_paths_score(ep)[0];
    const int64_t tl = dh_format_pair(name[0].c_str(), seq[0].data(), aoff[1], name[1].c_str(), seq[1].data(), boff[1], ops, nops, score,
                                      &sc, width, nullptr, 0);
    if (tl < 0) die(dh_last_error());
    std::vector<char> text((size_t)tl + 1);
    dh_format_pair(name[0].c_str(), seq[0].data(), aoff[1], name[1].c_str(), seq[1].data(), boff[1], ops, nops, score, &sc, width,
                   text.data(), tl + 1);
    FILE *o = outfile.empty() ? stdout : fopen(outfile.c_str(), "w");
    if (!o) die("cannot write " + outfile);
    const bool ok = fwrite(text.data(), 1, (size_t)tl, o) == (size_t)tl;
    if ((o != stdout ? fclose(o) : fflush(o)) != 0 || !ok) die("write error");
    dh_edit_paths_destroy(ep);
    dh_ctx_destroy(ctx);
    return 0;
}

// ---------------------------------------------------------------------------------- fm-index
// The contract is the reference program's (external/fm-index.cpp), restated: records and queries are lines; record ids are
// 0-based line numbers, empty lines included; empty query lines are skipped and do not advance the 0-based query id, which
// restarts for every source; per query all forward occurrences ascending by (record, begin), then with -r those of the
// reverse complement; coordinates 0-based, right-open, relative to the record.  Deviations: no index is built --
// <reference>.fm9 is a small file of our own that says so (check-results asserts that it exists, checkResults.d:684), and
// <reference>.idx is not written; a last line without '\n' is a record (the reference program throws on a hit in it);
// the alphabet is acgt, or ACGT if every letter of the reference and of all queries is upper case -- any other byte, or
// mixed case, ends the run (the reference program matches bytes, so nothing is case-folded silently).
namespace {
const char kFm9Magic[8] = {'d', 'h', 'f', 'm', '9', '\n', 0, 0};
const int64_t kFm9Version = 1;

struct FmLetters {  // the case of the first letter seen, and where
    int upper = -1;
    std::string file;
    long long line = 0;
};

// the lines of `text` as codes appended to `seq`, their ends to `off`; keep_empty: empty lines are records
void fm_lines(const std::string &text, const std::string &file, bool keep_empty, FmLetters &lt, std::vector<uint8_t> &seq,
              std::vector<int64_t> &off, std::vector<int64_t> *text_starts)
{
    long long line = 1;
    size_t p = 0;
    while (p < text.size()) {
        size_t eol = text.find('\n', p);
        const bool last_open = eol == std::string::npos;
        if (last_open) eol = text.size();
        if (text_starts) text_starts->push_back((int64_t)p);
        for (size_t k = p; k < eol; k++) {
            const unsigned char c = (unsigned char)text[k];
            const unsigned char l = (unsigned char)(c | 32);
            const bool letter = (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z');
            if (!letter || (l != 'a' && l != 'c' && l != 'g' && l != 't')) {
                char msg[256];
                snprintf(msg, sizeof(msg), "%s: line %lld: byte 0x%02x%s is not one of acgt (or ACGT)", file.c_str(), line, c,
                         c == 'n' || c == 'N' ? " (n)" : "");
                die(msg, 2);
            }
            const int upper = c < 'a';
            if (lt.upper < 0) {
                lt.upper = upper;
                lt.file = file;
                lt.line = line;
            } else if (lt.upper != upper) {
                char msg[512];
                snprintf(msg, sizeof(msg), "%s: line %lld: %s-case letter, but %s line %lld is %s case: bytes are matched as they are, mixed "
                         "case is refused", file.c_str(), line, upper ? "upper" : "lower", lt.file.c_str(), lt.line, lt.upper ? "upper" : "lower");
                die(msg, 2);
            }
            seq.push_back((uint8_t)(l == 'a' ? 0 : l == 'c' ? 1 : l == 'g' ? 2 : 3));
        }
        if (keep_empty || eol > p) off.push_back((int64_t)seq.size());
        p = eol + 1;
        line++;
    }
}

bool fm9_current(const std::string &path, int64_t size)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char magic[8];
    int64_t head[2] = {0, 0};
    const bool ok = fread(magic, 1, 8, f) == 8 && fread(head, 8, 2, f) == 2 && memcmp(magic, kFm9Magic, 8) == 0 &&
                    head[0] == kFm9Version && head[1] == size;
    fclose(f);
    return ok;
}
}  // namespace

static int tool_fm_index(const std::vector<std::string> &args)
{
    auto usage = [](const std::string &err) {
        fprintf(stderr,
                "error: %s\n\nUsage fm-index [-P<dir>] [-r] <in:reference> [<in:queries> ...]\n"
                "    Locates every exact occurrence of the <queries> (one per line) in <reference>\n"
                "    (one record per line) on the GPU; reads standard input if no <queries> is given.\n\n"
                "    -P<dir>   temporary directory (must exist; unused)\n"
                "    -r        search the reverse complement of each query as well\n\n"
                "    Output, TAB-separated: refName refId refLength queryId hitBegin hitEnd revComp\n"
                "    Ids and coordinates are zero-based, coordinates right-open.  Leaves <reference>.fm9.\n",
                err.c_str());
        return 1;
    };
    bool both = false;
    std::string tmpdir;
    size_t i = 0;
    for (; i < args.size() && !args[i].empty() && args[i][0] == '-'; i++) {
        const std::string &a = args[i];
        if (a.size() >= 2 && a[1] == 'P') {
            tmpdir = a.substr(2);
            if (tmpdir.empty()) return usage("Missing value for -P.");
        } else if (a == "-r")
            both = true;
        else if (a.size() >= 2 && a[1] == 'r')
            return usage("Flag -r takes no value.");
        else
            return usage("Invalid option " + a + ".");
    }
    if (!tmpdir.empty()) {
        struct stat sb;
        if (stat(tmpdir.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode)) return usage("Cannot open temporary directory: " + tmpdir);
    }
    if (i >= args.size()) return usage("Missing arguments.");
    const std::string ref_path = args[i];
    const std::vector<std::string> qfiles(args.begin() + (long)i + 1, args.end());
    // ---- the reference: records, alphabet, <reference>.fm9
    FILE *f = fopen(ref_path.c_str(), "rb");
    if (!f) die("File `" + ref_path + "` does not exist.", 2);
    const std::string ref_text = slurp(f);
    fclose(f);
    FmLetters lt;
    std::vector<uint8_t> rseq, qseq;
    std::vector<int64_t> roff{0}, qoff{0}, text_starts;
    fm_lines(ref_text, ref_path, true, lt, rseq, roff, &text_starts);
    text_starts.push_back((int64_t)ref_text.size());
    const int64_t nref = (int64_t)roff.size() - 1;
    const std::string fm9 = ref_path + ".fm9";
    if (!fm9_current(fm9, (int64_t)ref_text.size())) {
        fprintf(stderr, "{\"level\":\"info\",\"info\":\"Writing the record list (no index is needed).\",\"file\":\"%s\"}\n", fm9.c_str());
        FILE *o = fopen(fm9.c_str(), "wb");
        if (!o) die("cannot write " + fm9, 2);
        const int64_t head[3] = {kFm9Version, (int64_t)ref_text.size(), nref};
        const bool ok = fwrite(kFm9Magic, 1, 8, o) == 8 && fwrite(head, 8, 3, o) == 3 &&
                        fwrite(text_starts.data(), 8, text_starts.size(), o) == text_starts.size();
        if (fclose(o) != 0 || !ok) die("write error on " + fm9, 2);
    }
    // ---- the queries of every source
    struct Source {
        std::string name;
        int64_t first;  // its first query in the call
    };
    std::vector<Source> sources;
    auto add_source = [&](const std::string &name, const std::string &text) {
        sources.push_back(Source{name, (int64_t)qoff.size() - 1});
        fm_lines(text, name, false, lt, qseq, qoff, nullptr);
    };
    if (qfiles.empty())
        add_source("stdin", slurp(stdin));
    else
        for (const std::string &q : qfiles) {
            FILE *qf = fopen(q.c_str(), "rb");
            if (!qf) {
                fprintf(stderr, "{\"level\":\"warning\",\"info\":\"File does not exist. Skipping.\",\"file\":\"%s\"}\n", q.c_str());
                continue;
            }
            add_source(q, slurp(qf));
            fclose(qf);
        }
    const int64_t nqry = (int64_t)qoff.size() - 1;
    dh_ctx *ctx = nullptr;
    CHK(dh_ctx_create(0, nullptr, &ctx));
    dh_exact_hits *hits = nullptr;
    CHK(dh_exact_locate(ctx, rseq.data(), roff.data(), nref, qseq.data(), qoff.data(), nqry, both ? 1 : 0, &hits));
    const dh_exact_hit *h = dh_exact_hits_records(hits);
    const int64_t nh = dh_exact_hits_count(hits);
    size_t s = 0;
    std::string line;
    for (int64_t k = 0; k < nh; k++) {
        while (s + 1 < sources.size() && h[k].query >= sources[s + 1].first) s++;
        char buf[160];
        snprintf(buf, sizeof(buf), "\t%d\t%lld\t%lld\t%lld\t%lld\t%s\n", h[k].ref, (long long)(roff[(size_t)h[k].ref + 1] - roff[(size_t)h[k].ref]),
                 (long long)(h[k].query - sources[s].first), (long long)h[k].begin, (long long)h[k].end, h[k].complement ? "yes" : "no");
        line = sources[s].name + buf;
        if (fwrite(line.data(), 1, line.size(), stdout) != line.size()) die("write error", 2);
    }
    if (fflush(stdout) != 0) die("write error", 2);
    dh_exact_hits_destroy(hits);
    dh_ctx_destroy(ctx);
    return 0;
}

// ---------------------------------------------------------------------------------- chain-local-alignments
// Unknown options: the usage text and exit 1.  Everything else that fails: the library's message and exit 2.
static int tool_chain(const std::vector<std::string> &args)
{
    const char *usage = "usage: chain-local-alignments [--max-indel=<bps>] [--max-chain-gap=<bps>] [--max-relative-overlap=<f>] "
                        "[--min-relative-score=<f>] [--min-score=<n>] <ref-db> [<reads-db>] <in:las> <out:las>";
    auto fail = [](const std::string &what) {
        fprintf(stderr, "chain-local-alignments: %s\n", what.c_str());
        return 2;
    };
    std::vector<std::string> pos;
    std::string v_indel, v_gap, v_ovl, v_rel, v_min;
    for (const std::string &a : args) {
        auto value = [&](const char *name, std::string &out) {
            const size_t len = strlen(name);
            if (a.compare(0, len, name) != 0 || a.size() <= len) return false;
            out = a.substr(len);
            return true;
        };
        if (value("--max-indel=", v_indel) || value("--max-chain-gap=", v_gap) || value("--max-relative-overlap=", v_ovl) ||
            value("--min-relative-score=", v_rel) || value("--min-score=", v_min))
            continue;
        if (a.size() > 1 && a[0] == '-') die("unknown or malformed option " + a + "\n" + usage);
        pos.push_back(a);
    }
    if (pos.size() != 3 && pos.size() != 4) die(usage);
    const std::string &in = pos[pos.size() - 2], &out = pos[pos.size() - 1];
    dh_la_set *set = nullptr, *chained = nullptr;
    if (dh_las_read(in.c_str(), &set)) return fail(dh_last_error());
    dh_chain_opts o;
    dh_default_chain_opts(&o, dh_la_set_tspace(set));
    auto number = [&](const std::string &v, bool real, double *d, int32_t *i) {
        if (v.empty()) return true;
        char *end = nullptr;
        if (real)
            *d = strtod(v.c_str(), &end);
        else
            *i = (int32_t)strtol(v.c_str(), &end, 10);
        return end && *end == 0;
    };
    if (!number(v_indel, false, nullptr, &o.max_indel) || !number(v_gap, false, nullptr, &o.max_chain_gap) ||
        !number(v_min, false, nullptr, &o.min_score) || !number(v_ovl, true, &o.max_relative_overlap, nullptr) ||
        !number(v_rel, true, &o.min_relative_score, nullptr))
        return fail("an option's value is not a number");
    // the DBs only say which read ids exist
    dh_dazz *da = nullptr, *db = nullptr;
    if (dh_dazz_open(pos[0].c_str(), &da)) return fail(dh_last_error());
    if (pos.size() == 4 && dh_dazz_open(pos[1].c_str(), &db)) return fail(dh_last_error());
    const dh_dazz *dbz = db ? db : da;
    const int64_t n = dh_la_set_count(set);
    const dh_la *las = dh_la_set_records(set);
    for (int64_t i = 0; i < n; i++) {
        const int64_t a = (int64_t)las[i].aread - dh_dazz_first_id(da), b = (int64_t)las[i].bread - dh_dazz_first_id(dbz);
        if (a < 0 || a >= dh_dazz_nreads(da) || b < 0 || b >= dh_dazz_nreads(dbz))
            return fail("record " + std::to_string(i) + " of " + in + ": a read id outside the DB");
    }
    dh_ctx *ctx = nullptr;
    if (dh_ctx_create(0, nullptr, &ctx)) return fail(dh_last_error());
    dh_la_chains *chains = nullptr;
    if (dh_la_chain(ctx, las, n, &o, &chains)) return fail(dh_last_error());
    if (dh_la_chains_to_set(chains, las, n, dh_la_set_trace(set), dh_la_set_tspace(set), &chained)) return fail(dh_last_error());
    static const uint16_t no_trace = 0;
    const uint16_t *tr = dh_la_set_trace(chained);
    if (dh_las_write(out.c_str(), dh_la_set_records(chained), dh_la_set_count(chained), tr ? tr : &no_trace, dh_la_set_tspace(chained)))
        return fail(dh_last_error());
    dh_la_chains_destroy(chains);
    dh_la_set_destroy(chained);
    dh_la_set_destroy(set);
    if (db) dh_dazz_close(db);
    dh_dazz_close(da);
    dh_ctx_destroy(ctx);
    return 0;
}

// readMasks (propagateMask.d:136-142, collectPileUps/package.d:100-110): the union of the mask tracks `masks` of the opened DB,
// per contig sorted with intersecting or touching intervals merged.  Returns "" or what failed.
static std::string read_united_masks(const dh_dazz *da, const std::string &db_path, const std::vector<std::string> &masks,
                                     std::vector<int64_t> &mask_ptr, std::vector<int32_t> &mask_iv)
{
    const int32_t ncontigs = dh_dazz_nreads(da);
    std::vector<std::vector<std::pair<int32_t, int32_t>>> per((size_t)ncontigs);
    for (const std::string &m : masks) {
        std::vector<int64_t> ptr((size_t)ncontigs + 1);
        const int64_t cnt = dh_dazz_read_mask(da, db_path.c_str(), m.c_str(), ptr.data(), nullptr, 0);
        if (cnt < 0) return "mask " + m + ": " + dh_last_error();
        std::vector<int32_t> iv((size_t)(2 * cnt) + 2);
        if (dh_dazz_read_mask(da, db_path.c_str(), m.c_str(), ptr.data(), iv.data(), cnt) < 0) return "mask " + m + ": " + dh_last_error();
        for (int32_t c = 0; c < ncontigs; c++)
            for (int64_t j = ptr[(size_t)c]; j < ptr[(size_t)c + 1]; j++)
                if (iv[(size_t)(2 * j + 1)] > iv[(size_t)(2 * j)]) per[(size_t)c].push_back({iv[(size_t)(2 * j)], iv[(size_t)(2 * j + 1)]});
    }
    mask_ptr.assign(1, 0);
    mask_iv.clear();
    for (auto &v : per) {
        std::sort(v.begin(), v.end());
        size_t first = mask_iv.size();
        for (const auto &x : v) {
            if (mask_iv.size() > first && x.first <= mask_iv.back())
                mask_iv.back() = std::max(mask_iv.back(), x.second);
            else {
                mask_iv.push_back(x.first);
                mask_iv.push_back(x.second);
            }
        }
        mask_ptr.push_back((int64_t)mask_iv.size() / 2);
    }
    mask_iv.push_back(0);  // (never an empty array)
    return "";
}

// ---------------------------------------------------------------------------------- propagate-mask
// Unknown options: the usage text and exit 1.  Everything else that fails: the library's message and exit 2.
static int tool_propagate_mask(const std::vector<std::string> &args)
{
    const char *usage = "usage: propagate-mask -m <mask> [-m <mask>]... [--config=<file>] [-v] [--quiet] [-T<n>] <ref-db> [<reads-db>] "
                        "<db-alignment> <out-mask>";
    auto fail = [](const std::string &what) {
        fprintf(stderr, "propagate-mask: %s\n", what.c_str());
        return 2;
    };
    std::vector<std::string> pos, masks;
    bool ignored = false;
    for (size_t i = 0; i < args.size(); i++) {
        const std::string &a = args[i];
        if (a == "-m" && i + 1 < args.size())
            masks.push_back(args[++i]);
        else if (a.size() > 2 && a.compare(0, 2, "-m") == 0)
            masks.push_back(a.substr(2));
        else if (a.size() > 7 && a.compare(0, 7, "--mask=") == 0)
            masks.push_back(a.substr(7));
        else if (a == "-v" || a == "--quiet" || (a.size() > 9 && a.compare(0, 9, "--config=") == 0) ||
                 (a.size() > 2 && a.compare(0, 2, "-T") == 0) || (a.size() > 10 && a.compare(0, 10, "--threads=") == 0))
            ignored = true;
        else if (a.size() > 1 && a[0] == '-')
            die("unknown or malformed option " + a + "\n" + usage);
        else
            pos.push_back(a);
    }
    if (masks.empty() || (pos.size() != 3 && pos.size() != 4)) die(usage);
    if (ignored) fprintf(stderr, "propagate-mask: --config, -v, --quiet, -T and --threads have no effect here\n");
    const std::string &in = pos[pos.size() - 2], &out_name = pos[pos.size() - 1], &dest_path = pos.size() == 4 ? pos[1] : pos[0];
    dh_dazz *da = nullptr, *db = nullptr;
    if (dh_dazz_open(pos[0].c_str(), &da)) return fail(dh_last_error());
    if (pos.size() == 4 && dh_dazz_open(pos[1].c_str(), &db)) return fail(dh_last_error());
    const dh_dazz *dest = db ? db : da;
    const int32_t ncontigs = dh_dazz_nreads(da), nreads = dh_dazz_nreads(dest);
    std::vector<int64_t> mask_ptr;
    std::vector<int32_t> mask_iv;
    const std::string mask_err = read_united_masks(da, pos[0], masks, mask_ptr, mask_iv);
    if (!mask_err.empty()) return fail(mask_err);
    dh_la_set *set = nullptr;
    if (dh_las_read(in.c_str(), &set)) return fail(dh_last_error());
    const int64_t n = dh_la_set_count(set);
    std::vector<dh_la> las(dh_la_set_records(set), dh_la_set_records(set) + n);
    for (dh_la &l : las) {  // ids of the opened views
        l.aread -= dh_dazz_first_id(da);
        l.bread -= dh_dazz_first_id(dest);
    }
    dh_ctx *ctx = nullptr;
    if (dh_ctx_create(0, nullptr, &ctx)) return fail(dh_last_error());
    dh_mask_result *res = nullptr;
    if (dh_la_propagate_mask(ctx, las.data(), n, dh_la_set_trace(set), dh_la_set_trace_len(set), dh_la_set_tspace(set), mask_ptr.data(),
                             mask_iv.data(), ncontigs, dh_dazz_offsets(dest), nreads, &res))
        return fail(dh_last_error());
    static const int32_t no_iv[2] = {0, 0};
    const int32_t *iv = dh_mask_result_count(res) > 0 ? dh_mask_result_iv(res) : no_iv;
    if (dh_dazz_write_mask(dest_path.c_str(), out_name.c_str(), nreads, dh_mask_result_ptr(res), iv)) return fail(dh_last_error());
    dh_mask_result_destroy(res);
    dh_la_set_destroy(set);
    if (db) dh_dazz_close(db);
    dh_dazz_close(da);
    dh_ctx_destroy(ctx);
    return 0;
}

// ---------------------------------------------------------------------------------- validate-regions
// Unknown options: the usage text and exit 1.  Everything else that fails: the library's message and exit 2.
static int tool_validate_regions(const std::vector<std::string> &args)
{
    const char *usage = "usage: validate-regions [--min-coverage-reads=<n> | --read-coverage=<f> --ploidy=<n>] [--min-spanning-reads=<n>] "
                        "[--region-context=<bps>] [--weak-coverage-window=<bps>] [--weak-coverage-mask=<mask>] [--report-all] "
                        "[--config=<file>] [-v] [--quiet] [-T<n>] <ref-db> <reads-db> <in.las> <regions-mask>";
    auto fail = [](const std::string &what) {
        fprintf(stderr, "validate-regions: %s\n", what.c_str());
        return 2;
    };
    std::vector<std::string> pos;
    std::string v_min_cov, v_cov, v_ploidy, v_span, v_context, v_window, out_mask;
    bool ignored = false, report_all = false;
    auto value = [](const std::string &a, const char *key, std::string *out) {
        const size_t k = strlen(key);
        if (a.size() <= k || a.compare(0, k, key) != 0) return false;
        *out = a.substr(k);
        return true;
    };
    for (const std::string &a : args) {
        if (value(a, "--min-coverage-reads=", &v_min_cov) || value(a, "--read-coverage=", &v_cov) || value(a, "--ploidy=", &v_ploidy) ||
            value(a, "--min-spanning-reads=", &v_span) || value(a, "--region-context=", &v_context) ||
            value(a, "--weak-coverage-window=", &v_window) || value(a, "--weak-coverage-mask=", &out_mask))
            continue;
        if (a == "--report-all")
            report_all = true;
        else if (a == "-v" || a == "--quiet" || (a.size() > 9 && a.compare(0, 9, "--config=") == 0) ||
                 (a.size() > 2 && a.compare(0, 2, "-T") == 0) || (a.size() > 10 && a.compare(0, 10, "--threads=") == 0))
            ignored = true;
        else if (a.size() > 1 && a[0] == '-')
            die("unknown or malformed option " + a + "\n" + usage);
        else
            pos.push_back(a);
    }
    if (pos.size() != 4) die(usage);
    if (ignored) fprintf(stderr, "validate-regions: --config, -v, --quiet, -T and --threads have no effect here\n");
    // the defaults of commandline.d:2187, 2411, 2497; the coverage options of :2060-2088
    int32_t min_cov = 0, min_span = 3, context = 1000, window = 500, ploidy = 0;
    double read_cov = 0;
    auto number = [](const std::string &v, bool real, double *d, int32_t *i) {
        if (v.empty()) return true;
        char *end = nullptr;
        if (real)
            *d = strtod(v.c_str(), &end);
        else
            *i = (int32_t)strtol(v.c_str(), &end, 10);
        return end && *end == 0;
    };
    if (!number(v_min_cov, false, nullptr, &min_cov) || !number(v_cov, true, &read_cov, nullptr) || !number(v_ploidy, false, nullptr, &ploidy) ||
        !number(v_span, false, nullptr, &min_span) || !number(v_context, false, nullptr, &context) || !number(v_window, false, nullptr, &window))
        return fail("an option's value is not a number");
    if (v_min_cov.empty() == v_cov.empty()) return fail("exactly one of --min-coverage-reads and --read-coverage must be given");
    if (!v_cov.empty()) {
        if (ploidy <= 0) return fail("--read-coverage needs --ploidy > 0");
        min_cov = (int32_t)(0.5 * read_cov / ploidy);
    }
    dh_dazz *da = nullptr, *db = nullptr;
    if (dh_dazz_open(pos[0].c_str(), &da)) return fail(dh_last_error());
    if (dh_dazz_open(pos[1].c_str(), &db)) return fail(dh_last_error());
    const int32_t ncontigs = dh_dazz_nreads(da);
    dh_la_set *set = nullptr;
    if (dh_las_read(pos[2].c_str(), &set)) return fail(dh_last_error());
    const int64_t n = dh_la_set_count(set);
    if (n == 0) {  // (:151-159)
        fprintf(stderr, "validate-regions: warning: empty reads-alignment %s\n", pos[2].c_str());
        return 0;
    }
    std::vector<dh_la> las(dh_la_set_records(set), dh_la_set_records(set) + n);
    for (dh_la &l : las) {  // ids of the opened views
        l.aread -= dh_dazz_first_id(da);
        l.bread -= dh_dazz_first_id(db);
    }
    // the regions of the contigs between the first and the last aread of the file (:259-271)
    std::vector<int64_t> ptr((size_t)ncontigs + 1);
    const int64_t cnt = dh_dazz_read_mask(da, pos[0].c_str(), pos[3].c_str(), ptr.data(), nullptr, 0);
    if (cnt < 0) return fail("mask " + pos[3] + ": " + dh_last_error());
    std::vector<int32_t> iv((size_t)(2 * cnt) + 2);
    if (dh_dazz_read_mask(da, pos[0].c_str(), pos[3].c_str(), ptr.data(), iv.data(), cnt) < 0) return fail("mask " + pos[3] + ": " + dh_last_error());
    std::vector<dh_region> regions;
    for (int32_t c = std::max(0, las.front().aread); c < ncontigs && c <= las.back().aread; c++)
        for (int64_t j = ptr[(size_t)c]; j < ptr[(size_t)c + 1]; j++) regions.push_back(dh_region{c, iv[(size_t)(2 * j)], iv[(size_t)(2 * j + 1)]});
    dh_ctx *ctx = nullptr;
    if (dh_ctx_create(0, nullptr, &ctx)) return fail(dh_last_error());
    dh_region_result *res = nullptr;
    if (dh_la_validate_regions(ctx, las.data(), n, dh_dazz_offsets(da), ncontigs, regions.data(), (int32_t)regions.size(), context, window,
                               min_cov, min_span, &res))
        return fail(dh_last_error());
    const dh_region_report *rep = dh_region_result_reports(res);
    const int64_t *span_off = dh_region_result_span_off(res);
    const int32_t *span_ids = dh_region_result_span_ids(res);
    const int32_t first_contig = dh_dazz_first_id(da) + 1, first_read = dh_dazz_first_id(db) + 1;  // the ids of the report are 1-based
    for (size_t r = 0; r < regions.size(); r++) {
        if (rep[r].is_valid && !report_all) continue;
        printf("{\"region\":{\"contigId\":%d,\"begin\":%d,\"end\":%d},\"regionWithContext\":{\"contigId\":%d,\"begin\":%d,\"end\":%d},"
               "\"isValid\":%s,\"numSpanningReads\":%d,\"spanningReadIds\":[",
               regions[r].contig + first_contig, regions[r].begin, regions[r].end, regions[r].contig + first_contig, rep[r].ctx_begin,
               rep[r].ctx_end, rep[r].is_valid ? "true" : "false", rep[r].num_spanning_reads);
        for (int64_t k = span_off[r]; k < span_off[r + 1]; k++) printf("%s%d", k > span_off[r] ? "," : "", span_ids[k] + first_read);
        printf("],\"weakCoverageMaskBps\":%d}\n", rep[r].weak_bp);
    }
    if (!out_mask.empty()) {
        static const int32_t no_iv[2] = {0, 0};
        const int32_t *miv = dh_region_result_mask_count(res) > 0 ? dh_region_result_mask_iv(res) : no_iv;
        if (dh_dazz_write_mask(pos[0].c_str(), out_mask.c_str(), ncontigs, dh_region_result_mask_ptr(res), miv)) return fail(dh_last_error());
    }
    dh_region_result_destroy(res);
    dh_la_set_destroy(set);
    dh_dazz_close(db);
    dh_dazz_close(da);
    dh_ctx_destroy(ctx);
    return 0;
}

// ---------------------------------------------------------------------------------- collect
// `dentist collect` (collectPileUps/package.d:88-206): the six alignment filters on the device, the scaffold graph with
// resolveBubbles, every pile-up written to <pile-ups.db>.  Unknown options: the usage text and exit 1.  Everything else that
// fails: the library's message and exit 2.
static int tool_collect(const std::vector<std::string> &args)
{
    const char *usage = "usage: collect [--mask=<name>[,<name>...]]... [--max-alignment-error=<f>] [--min-anchor-length=<n>] "
                        "[--proper-alignment-allowance=<n>] [--min-spanning-reads=<n>] [--best-pile-up-margin=<f>] "
                        "[--existing-gap-bonus=<f>] [--no-merge-extension] <ref-db> <reads-db> <ref-vs-reads.las> <pile-ups.db>";
    auto fail = [](const std::string &what) {
        fprintf(stderr, "collect: %s\n", what.c_str());
        return 2;
    };
    std::vector<std::string> pos, masks;
    std::string v_err, v_anchor, v_allow, v_span, v_margin, v_bonus, unused;
    bool ignored = false, merge_extensions = true;
    auto value = [](const std::string &a, const char *key, std::string *out) {
        const size_t k = strlen(key);
        if (a.size() <= k || a.compare(0, k, key) != 0) return false;
        *out = a.substr(k);
        return true;
    };
    auto add_masks = [&](const std::string &list) {  // <name>[,<name>...]
        size_t at = 0;
        while (at <= list.size()) {
            const size_t comma = std::min(list.find(',', at), list.size());
            if (comma > at) masks.push_back(list.substr(at, comma - at));
            at = comma + 1;
        }
    };
    for (size_t i = 0; i < args.size(); i++) {
        const std::string &a = args[i];
        std::string v;
        if ((a == "-m" || a == "-e") && i + 1 < args.size()) {
            if (a == "-m")
                add_masks(args[++i]);
            else
                v_err = args[++i];
        } else if (value(a, "--mask=", &v) || (a.compare(0, 2, "--") != 0 && value(a, "-m", &v)))
            add_masks(v);
        else if (value(a, "--max-alignment-error=", &v_err) || (a.compare(0, 2, "--") != 0 && value(a, "-e", &v_err)) ||
                 value(a, "--min-anchor-length=", &v_anchor) || value(a, "--proper-alignment-allowance=", &v_allow) ||
                 value(a, "--min-spanning-reads=", &v_span) || value(a, "--best-pile-up-margin=", &v_margin) ||
                 value(a, "--existing-gap-bonus=", &v_bonus))
            continue;
        else if (a == "--no-merge-extension")
            merge_extensions = false;
        else if (a == "-v" || a == "--quiet" || value(a, "--config=", &unused) || value(a, "--threads=", &unused) ||
                 value(a, "--auxiliary-threads=", &unused) || value(a, "--tmpdir=", &unused) || value(a, "--damapper-ref-vs-reads=", &unused) ||
                 (a.compare(0, 2, "--") != 0 && (value(a, "-T", &unused) || value(a, "-A", &unused) || value(a, "-P", &unused))))
            ignored = true;
        else if (a.size() > 1 && a[0] == '-')
            die("unknown or malformed option " + a + "\n" + usage);
        else
            pos.push_back(a);
    }
    if (masks.empty() || pos.size() != 4) die(usage);  // (at least one mask: commandline.d:1789)
    if (ignored)
        fprintf(stderr, "collect: --config, -v, --quiet, -T / --threads, -A / --auxiliary-threads, -P / --tmpdir and --damapper-ref-vs-reads have "
                        "no effect here\n");
    dh_la_set *set = nullptr;
    if (dh_las_read(pos[2].c_str(), &set)) return fail(dh_last_error());
    const int64_t n = dh_la_set_count(set);
    if (n == 0) return fail("empty ref vs. reads alignment");  // (:127)
    const int32_t tspace = dh_la_set_tspace(set);
    // the defaults of commandline.d:1336, 1681, 1799-1808, 2024-2036, 2183, 2317-2332
    double max_err = 0.3;
    int32_t min_anchor = 500, allowance = tspace;
    dh_scaffold_opts so;
    dh_default_scaffold_opts(&so);
    so.min_spanning_reads = 3, so.best_pile_up_margin = 3.0, so.existing_gap_bonus = 6.0, so.merge_extensions = merge_extensions ? 1 : 0;
    auto number = [](const std::string &v, bool real, double *d, int32_t *i) {
        if (v.empty()) return true;
        char *end = nullptr;
        if (real)
            *d = strtod(v.c_str(), &end);
        else
            *i = (int32_t)strtol(v.c_str(), &end, 10);
        return end && *end == 0;
    };
    if (!number(v_err, true, &max_err, nullptr) || !number(v_anchor, false, nullptr, &min_anchor) || !number(v_allow, false, nullptr, &allowance) ||
        !number(v_span, false, nullptr, &so.min_spanning_reads) || !number(v_margin, true, &so.best_pile_up_margin, nullptr) ||
        !number(v_bonus, true, &so.existing_gap_bonus, nullptr))
        return fail("an option's value is not a number");
    if (!(max_err > 0 && max_err <= 0.3)) return fail("--max-alignment-error must lie in (0, 0.3]");
    dh_dazz *da = nullptr, *db = nullptr;
    if (dh_dazz_open(pos[0].c_str(), &da)) return fail(dh_last_error());
    if (dh_dazz_open(pos[1].c_str(), &db)) return fail(dh_last_error());
    const int32_t ncontigs = dh_dazz_nreads(da), nreads = dh_dazz_nreads(db);
    std::vector<int64_t> mask_ptr;
    std::vector<int32_t> mask_iv;
    const std::string mask_err = read_united_masks(da, pos[0], masks, mask_ptr, mask_iv);
    if (!mask_err.empty()) return fail(mask_err);
    std::vector<dh_la> las(dh_la_set_records(set), dh_la_set_records(set) + n);
    for (dh_la &l : las) {  // ids of the opened views
        l.aread -= dh_dazz_first_id(da);
        l.bread -= dh_dazz_first_id(db);
    }
    dh_ctx *ctx = nullptr;
    if (dh_ctx_create(0, nullptr, &ctx)) return fail(dh_last_error());
    dh_process_opts po;
    dh_default_process_opts(&po);
    po.max_align_err_ppm = (int32_t)llround(max_err * 1e6), po.allowance = allowance, po.min_anchor = min_anchor;
    int64_t dropped[6];
    if (dh_la_collect_filter(ctx, las.data(), n, dh_dazz_offsets(da), ncontigs, dh_dazz_offsets(db), nreads, mask_ptr.data(), mask_iv.data(), &po,
                             dropped, nullptr))
        return fail(dh_last_error());
    static const char *const stage[6] = {"LQ", "Improper", "WeaklyAnchored", "Contained", "Ambiguous", "Redundant"};
    for (int k = 0; k < 6; k++) fprintf(stderr, "collect: filter %s dropped %lld alignment chains\n", stage[k], (long long)dropped[k]);
    int64_t left = 0;
    for (const dh_la &l : las) left += l.flags & DH_FLAG_DISABLED ? 0 : 1;
    if (left == 0) return fail("no alignment chains left after filtering");  // (:153-156)
    // the gaps of the input assembly: contigs that follow each other in one scaffold of the .dam (getScaffoldStructure)
    std::vector<int32_t> gaps;
    for (int32_t c = 0; c + 1 < ncontigs; c++)
        if (dh_dazz_origin(da)[c + 1] > dh_dazz_origin(da)[c] && strcmp(dh_dazz_header(da, c), dh_dazz_header(da, c + 1)) == 0) {
            gaps.push_back(c);
            gaps.push_back(c + 1);
        }
    dh_db *A = nullptr, *B = nullptr;
    if (dh_db_create(ctx, dh_dazz_bases(da), dh_dazz_offsets(da), ncontigs, nullptr, &A)) return fail(dh_last_error());
    if (dh_db_create(ctx, dh_dazz_bases(db), dh_dazz_offsets(db), nreads, nullptr, &B)) return fail(dh_last_error());
    dh_align_opts ao;
    dh_default_align_opts(&ao);
    ao.tspace = tspace;
    dh_scaffold *sc = nullptr;
    dh_la_set *extra = nullptr;
    if (dh_scaffold_pileups_resolved(ctx, A, B, las.data(), n, gaps.data(), (int32_t)gaps.size() / 2, &so, &ao, allowance, 0, 0, &sc, &extra,
                                     nullptr))
        return fail(dh_last_error());
    // the records and traces of *extra behind the file's: LA index n + i is record i of *extra
    std::vector<uint16_t> trace(dh_la_set_trace(set), dh_la_set_trace(set) + dh_la_set_trace_len(set));
    const int64_t nx = extra ? dh_la_set_count(extra) : 0;
    for (int64_t i = 0; i < nx; i++) {
        dh_la l = dh_la_set_records(extra)[i];
        l.toff += (int64_t)trace.size();
        las.push_back(l);
    }
    if (nx) trace.insert(trace.end(), dh_la_set_trace(extra), dh_la_set_trace(extra) + dh_la_set_trace_len(extra));
    dh_pileups *piles = nullptr;
    if (dh_scaffold_all_pileups(sc, las.data(), (int64_t)las.size(), 3, &piles, nullptr)) return fail(dh_last_error());
    trace.push_back(0);  // (never an empty array)
    if (dh_pileups_write_db(piles, las.data(), (int64_t)las.size(), trace.data(), dh_dazz_offsets(da), ncontigs, dh_dazz_offsets(db), nreads,
                            tspace, pos[3].c_str()))
        return fail(dh_last_error());
    dh_pileups_destroy(piles);
    if (extra) dh_la_set_destroy(extra);
    dh_scaffold_destroy(sc);
    dh_db_destroy(B);
    dh_db_destroy(A);
    dh_la_set_destroy(set);
    dh_dazz_close(db);
    dh_dazz_close(da);
    dh_ctx_destroy(ctx);
    return 0;
}

// ---------------------------------------------------------------------------------- mask-repetitive-regions
// Unknown options and the reference's option validation (commandline.d:1840-1972): the message and exit 1.  Everything else that
// fails: the library's message and exit 2.
static int tool_mask_repetitive_regions(const std::vector<std::string> &args)
{
    const std::string usage = "usage: mask-repetitive-regions [--read-coverage=<f> | --max-coverage-reads=<n>] [--max-improper-coverage-reads=<n>] "
                              "[--max-coverage-self=<n>] [--proper-alignment-allowance=<n>] [--debug-repeat-masks] [--config=<file>] [-v] "
                              "[--quiet] [-T<n>] <ref-db> [<reads-db>] <db-alignment> <repeat-mask>";
    auto fail = [](const std::string &what) {
        fprintf(stderr, "mask-repetitive-regions: %s\n", what.c_str());
        return 2;
    };
    std::vector<std::string> pos;
    bool ignored = false, debug_masks = false, has_cov = false, has_max = false, has_max_improper = false, has_allowance = false;
    double read_coverage = 0.0;
    long long max_reads = 0, max_improper = 0, max_self = 4, allowance = 0;
    auto number = [&](const std::string &a, size_t at, long long *out) {
        char *end = nullptr;
        *out = strtoll(a.c_str() + at, &end, 10);
        if (end == a.c_str() + at || *end || *out < 0 || *out > INT32_MAX) die("unknown or malformed option " + a + "\n" + usage);
    };
    auto starts = [](const std::string &a, const char *p) { return a.size() > strlen(p) && a.compare(0, strlen(p), p) == 0; };
    for (const std::string &a : args) {
        if (starts(a, "--read-coverage=")) {
            char *end = nullptr;
            read_coverage = strtod(a.c_str() + 16, &end);
            if (end == a.c_str() + 16 || *end || !(read_coverage > 0.0)) die("unknown or malformed option " + a + "\n" + usage);
            has_cov = true;
        } else if (starts(a, "--max-coverage-reads="))
            number(a, 21, &max_reads), has_max = true;
        else if (starts(a, "--max-improper-coverage-reads="))
            number(a, 30, &max_improper), has_max_improper = true;
        else if (starts(a, "--max-coverage-self="))
            number(a, 20, &max_self);
        else if (starts(a, "--proper-alignment-allowance="))
            number(a, 29, &allowance), has_allowance = true;
        else if (a == "--debug-repeat-masks")
            debug_masks = true;
        else if (a == "-v" || a == "--quiet" || starts(a, "--config=") || starts(a, "-T") || starts(a, "--threads="))
            ignored = true;
        else if (a.size() > 1 && a[0] == '-')
            die("unknown or malformed option " + a + "\n" + usage);
        else
            pos.push_back(a);
    }
    if (pos.size() != 3 && pos.size() != 4) die(usage);
    const bool reads_case = pos.size() == 4;
    if (reads_case) {  // commandline.d:1868-1875, 1948-1955
        if (!has_max && !has_cov) die("must provide either --read-coverage or --max-coverage-reads");
        if (has_max && has_cov) die("must not provide both --read-coverage and --max-coverage-reads");
        if (!has_max_improper && !has_cov) die("must provide either --read-coverage or --max-improper-coverage-reads");
        if (has_max_improper && has_cov) die("must not provide both --read-coverage and --max-improper-coverage-reads");
    } else if (max_self < 1)
        die("--max-coverage-self must be positive");
    if (ignored) fprintf(stderr, "mask-repetitive-regions: --config, -v, --quiet, -T and --threads have no effect here\n");
    const std::string &in = pos[pos.size() - 2], &out_name = pos[pos.size() - 1];
    dh_dazz *da = nullptr, *db = nullptr;
    if (dh_dazz_open(pos[0].c_str(), &da)) return fail(dh_last_error());
    if (reads_case && dh_dazz_open(pos[1].c_str(), &db)) return fail(dh_last_error());
    const dh_dazz *other = db ? db : da;  // (a self alignment has the contigs on both sides)
    const int32_t ncontigs = dh_dazz_nreads(da), nreads = dh_dazz_nreads(other);
    dh_la_set *set = nullptr;
    if (dh_las_read(in.c_str(), &set)) return fail(dh_last_error());
    const int64_t n = dh_la_set_count(set);
    if (n == 0) fprintf(stderr, "mask-repetitive-regions: warning: empty %s-alignment\n", reads_case ? "reads" : "self");
    std::vector<dh_la> las(dh_la_set_records(set), dh_la_set_records(set) + n);
    for (dh_la &l : las) {  // ids of the opened views
        l.aread -= dh_dazz_first_id(da);
        l.bread -= dh_dazz_first_id(other);
    }
    dh_repeat_opts o;
    o.lower = 0, o.improper_lower = 0, o.with_improper = reads_case ? 1 : 0;
    o.upper = reads_case ? (has_cov ? dh_max_coverage_reads(read_coverage) : (int32_t)max_reads) : (int32_t)max_self;
    o.improper_upper = reads_case ? (has_cov ? dh_max_improper_coverage_reads(read_coverage) : (int32_t)max_improper) : 0;
    o.allowance = has_allowance ? (int32_t)allowance : dh_la_set_tspace(set);
    dh_ctx *ctx = nullptr;
    dh_repeat_result *res = nullptr;
    if (n > 0 && dh_ctx_create(0, nullptr, &ctx)) return fail(dh_last_error());
    static const int32_t no_iv[2] = {0, 0};
    if (n > 0) {
        if (dh_la_repeat_mask(ctx, las.data(), n, dh_dazz_offsets(da), ncontigs, dh_dazz_offsets(other), nreads, &o, &res)) return fail(dh_last_error());
        auto write = [&](const std::string &name, const int64_t *ptr, const int32_t *iv, int64_t count) {
            return dh_dazz_write_mask(pos[0].c_str(), name.c_str(), ncontigs, ptr, count > 0 ? iv : no_iv);
        };
        if (write(out_name, dh_repeat_result_mask_ptr(res), dh_repeat_result_mask_iv(res), dh_repeat_result_mask_count(res)))
            return fail(dh_last_error());
        if (debug_masks && reads_case) {  // maskRepetitiveRegions.d:225-237
            if (write(out_name + "-all", dh_repeat_result_all_ptr(res), dh_repeat_result_all_iv(res), dh_repeat_result_all_count(res)) ||
                write(out_name + "-improper", dh_repeat_result_improper_ptr(res), dh_repeat_result_improper_iv(res),
                      dh_repeat_result_improper_count(res)))
                return fail(dh_last_error());
        }
        dh_repeat_result_destroy(res);
    } else {  // an empty mask, without a device
        const std::vector<int64_t> ptr((size_t)ncontigs + 1, 0);
        if (dh_dazz_write_mask(pos[0].c_str(), out_name.c_str(), ncontigs, ptr.data(), no_iv)) return fail(dh_last_error());
        if (debug_masks && reads_case)
            if (dh_dazz_write_mask(pos[0].c_str(), (out_name + "-all").c_str(), ncontigs, ptr.data(), no_iv) ||
                dh_dazz_write_mask(pos[0].c_str(), (out_name + "-improper").c_str(), ncontigs, ptr.data(), no_iv))
                return fail(dh_last_error());
    }
    dh_la_set_destroy(set);
    if (db) dh_dazz_close(db);
    dh_dazz_close(da);
    if (ctx) dh_ctx_destroy(ctx);
    return 0;
}

// ---------------------------------------------------------------------------------- merge-masks, filter-mask
// Mask track `name` of the whole DB `da` as ptr / iv (iv never an empty array).  `<block>.<mask>` with a block of the DB names
// the track of that block (Snakefile:583-584): its reads are shifted by the block's first id into the whole DB's contig range.
// Returns "" or what failed.
static std::string read_mask_track(const dh_dazz *da, const std::string &db_path, const std::string &name, std::vector<int64_t> &ptr,
                                   std::vector<int32_t> &iv)
{
    const int32_t ncontigs = dh_dazz_nreads(da);
    ptr.assign((size_t)ncontigs + 1, 0);
    const int64_t cnt = dh_dazz_read_mask(da, db_path.c_str(), name.c_str(), ptr.data(), nullptr, 0);
    if (cnt < 0) return "mask " + name + ": " + dh_last_error();
    iv.assign((size_t)(2 * cnt) + 2, 0);
    if (dh_dazz_read_mask(da, db_path.c_str(), name.c_str(), ptr.data(), iv.data(), cnt) < 0) return "mask " + name + ": " + dh_last_error();
    const size_t dot = name.find('.');
    if (dot == std::string::npos || dot == 0 || name.find_first_not_of("0123456789") != dot) return "";
    const DbPath d = parse_db_path(db_path);
    const int32_t block = atoi(name.c_str());
    if (block < 1 || block > stub_blocks(d)) return "";
    dh_dazz *blk = nullptr;  // opened as TANmask opens the block of its .las
    if (dh_dazz_open((d.dir + "/" + d.root + "." + std::to_string(block) + "." + d.ext).c_str(), &blk)) return "mask " + name + ": " + dh_last_error();
    const int32_t first = dh_dazz_first_id(blk) - dh_dazz_first_id(da), nb = dh_dazz_nreads(blk);
    dh_dazz_close(blk);
    if (first < 0 || first + nb > ncontigs) return "mask " + name + ": the block lies outside the DB";
    const std::vector<int64_t> in(ptr);  // (entries 0 .. nb: the block's reads)
    for (int32_t c = 0; c <= ncontigs; c++) ptr[(size_t)c] = c < first ? 0 : in[(size_t)std::min(c - first, nb)];
    return "";
}

// the options both commands take and ignore; an unknown one: the usage and exit 1
static bool maskops_common_option(const std::string &a, bool *ignored)
{
    auto starts = [&](const char *p) { return a.size() > strlen(p) && a.compare(0, strlen(p), p) == 0; };
    if (a == "-v" || a == "--quiet" || starts("--config=") || starts("-T") || starts("--threads=")) {
        *ignored = true;
        return true;
    }
    return false;
}

// `dentist merge-masks` (commands/mergeMasks.d:47-53): the union of the input masks.  Everything that fails behind the options:
// the library's message and exit 2.
static int tool_merge_masks(const std::vector<std::string> &args)
{
    const std::string usage = "usage: merge-masks [--config=<file>] [-v] [--quiet] [-T<n>] <ref-db> <merged-mask> <input-mask>...";
    auto fail = [](const std::string &what) {
        fprintf(stderr, "merge-masks: %s\n", what.c_str());
        return 2;
    };
    std::vector<std::string> pos;
    bool ignored = false;
    for (const std::string &a : args) {
        if (maskops_common_option(a, &ignored)) continue;
        if (a.size() > 1 && a[0] == '-') die("unknown option " + a + "\n" + usage);
        pos.push_back(a);
    }
    if (pos.size() < 3) die(usage);
    if (ignored) fprintf(stderr, "merge-masks: --config, -v, --quiet, -T and --threads have no effect here\n");
    dh_dazz *da = nullptr;
    if (dh_dazz_open(pos[0].c_str(), &da)) return fail(dh_last_error());
    const int32_t ncontigs = dh_dazz_nreads(da), nmasks = (int32_t)pos.size() - 2;
    std::vector<std::vector<int64_t>> ptr((size_t)nmasks);
    std::vector<std::vector<int32_t>> iv((size_t)nmasks);
    std::vector<const int64_t *> pp;
    std::vector<const int32_t *> pi;
    for (int32_t k = 0; k < nmasks; k++) {
        const std::string err = read_mask_track(da, pos[0], pos[(size_t)k + 2], ptr[(size_t)k], iv[(size_t)k]);
        if (!err.empty()) return fail(err);
        pp.push_back(ptr[(size_t)k].data()), pi.push_back(iv[(size_t)k].data());
    }
    dh_ctx *ctx = nullptr;
    dh_mask_set *res = nullptr;
    dh_mask_opts o;
    dh_default_mask_opts(&o);
    if (dh_ctx_create(0, nullptr, &ctx)) return fail(dh_last_error());
    if (dh_mask_combine(ctx, pp.data(), pi.data(), nmasks, nullptr, nullptr, dh_dazz_offsets(da), ncontigs, &o, &res)) return fail(dh_last_error());
    static const int32_t no_iv[2] = {0, 0};
    if (dh_dazz_write_mask(pos[0].c_str(), pos[1].c_str(), ncontigs, dh_mask_set_ptr(res), dh_mask_set_count(res) > 0 ? dh_mask_set_iv(res) : no_iv))
        return fail(dh_last_error());
    dh_mask_set_destroy(res);
    dh_ctx_destroy(ctx);
    dh_dazz_close(da);
    return 0;
}

// `dentist filter-mask` (commands/filterMask.d:124-159): gaps up to --min-gap-size closed, then intervals below
// --min-interval-size dropped.  An empty input mask gives an empty mask (the reference indexes an empty array there).
static int tool_filter_mask(const std::vector<std::string> &args)
{
    const std::string usage = "usage: filter-mask [--min-gap-size=<n>] [--min-interval-size=<n>] [--config=<file>] [-v] [--quiet] [-T<n>] "
                              "<ref-db> <in-mask> <out-mask>";
    auto fail = [](const std::string &what) {
        fprintf(stderr, "filter-mask: %s\n", what.c_str());
        return 2;
    };
    std::vector<std::string> pos;
    bool ignored = false;
    long long min_gap = 0, min_interval = 0;
    auto number = [&](const std::string &a, size_t at, long long *out) {
        char *end = nullptr;
        *out = strtoll(a.c_str() + at, &end, 10);
        if (end == a.c_str() + at || *end || *out < 0 || *out > INT32_MAX) die("unknown or malformed option " + a + "\n" + usage);
    };
    for (const std::string &a : args) {
        if (a.compare(0, 15, "--min-gap-size=") == 0)
            number(a, 15, &min_gap);
        else if (a.compare(0, 20, "--min-interval-size=") == 0)
            number(a, 20, &min_interval);
        else if (maskops_common_option(a, &ignored))
            continue;
        else if (a.size() > 1 && a[0] == '-')
            die("unknown option " + a + "\n" + usage);
        else
            pos.push_back(a);
    }
    if (pos.size() != 3) die(usage);
    if (ignored) fprintf(stderr, "filter-mask: --config, -v, --quiet, -T and --threads have no effect here\n");
    dh_dazz *da = nullptr;
    if (dh_dazz_open(pos[0].c_str(), &da)) return fail(dh_last_error());
    const int32_t ncontigs = dh_dazz_nreads(da);
    std::vector<int64_t> ptr;
    std::vector<int32_t> iv;
    const std::string err = read_mask_track(da, pos[0], pos[1], ptr, iv);
    if (!err.empty()) return fail(err);
    static const int32_t no_iv[2] = {0, 0};
    if (ptr[(size_t)ncontigs] == 0) {  // an empty mask, without a device
        if (dh_dazz_write_mask(pos[0].c_str(), pos[2].c_str(), ncontigs, ptr.data(), no_iv)) return fail(dh_last_error());
        dh_dazz_close(da);
        return 0;
    }
    dh_ctx *ctx = nullptr;
    dh_mask_set *res = nullptr;
    const dh_mask_opts o{1, (int32_t)min_gap, (int32_t)min_interval, 0};
    const int64_t *pp = ptr.data();
    const int32_t *pi = iv.data();
    if (dh_ctx_create(0, nullptr, &ctx)) return fail(dh_last_error());
    if (dh_mask_combine(ctx, &pp, &pi, 1, nullptr, nullptr, dh_dazz_offsets(da), ncontigs, &o, &res)) return fail(dh_last_error());
    if (dh_dazz_write_mask(pos[0].c_str(), pos[2].c_str(), ncontigs, dh_mask_set_ptr(res), dh_mask_set_count(res) > 0 ? dh_mask_set_iv(res) : no_iv))
        return fail(dh_last_error());
    dh_mask_set_destroy(res);
    dh_ctx_destroy(ctx);
    dh_dazz_close(da);
    return 0;
}

// ---------------------------------------------------------------------------------- check-results
// `dentist check-results` (commands/checkResults.d), the subset tools/README.md states: the input contigs are placed in the result
// by exact search (dh_exact_locate, findReferenceContigs :399-565), every gap goes through dh_check_gaps, and the stats that need
// only the mask, the DB lengths, the mappings and the summaries are printed.  Everything that fails behind the options: the
// library's message and exit 2.
static int tool_check_results(const std::vector<std::string> &args)
{
    const std::string usage = "usage: check-results [--crop-alignment=<n>] [--crop-ambiguous=<n>] [--dust=<mask>] [--gap-details=<json>] "
                              "[--gap-details-context=0] [--json] [--config=<file>] [-v] [--quiet] [-T<n>] "
                              "<true-assembly> <mapped-regions-mask> <reference> <result>";
    auto fail = [](const std::string &what) {
        fprintf(stderr, "check-results: %s\n", what.c_str());
        return 2;
    };
    std::vector<std::string> pos;
    bool ignored = false, json = false, dust_given = false;
    long long crop = 0, crop_amb = 100, context = 0;
    std::string dust_name = "dust", details;
    auto number = [&](const std::string &a, size_t at, long long *out) {
        char *end = nullptr;
        *out = strtoll(a.c_str() + at, &end, 10);
        if (end == a.c_str() + at || *end || *out < 0 || *out > INT32_MAX) die("unknown or malformed option " + a + "\n" + usage);
    };
    for (const std::string &a : args) {
        if (a.compare(0, 17, "--crop-alignment=") == 0)
            number(a, 17, &crop);
        else if (a.compare(0, 17, "--crop-ambiguous=") == 0)
            number(a, 17, &crop_amb);
        else if (a.compare(0, 22, "--gap-details-context=") == 0)
            number(a, 22, &context);
        else if (a.compare(0, 7, "--dust=") == 0 && a.size() > 7)
            dust_name = a.substr(7), dust_given = true;
        else if (a.compare(0, 14, "--gap-details=") == 0 && a.size() > 14)
            details = a.substr(14);
        else if (a == "--json" || a == "-j")
            json = true;
        else if (maskops_common_option(a, &ignored))
            continue;
        else if (a.size() > 1 && a[0] == '-')
            die("unknown option " + a + "\n" + usage);
        else
            pos.push_back(a);
    }
    if (pos.size() != 4) die(usage);
    if (crop > crop_amb) die("--crop-alignment must be <= --crop-ambiguous\n" + usage);
    if (context != 0) die("--gap-details-context: only 0 is served (the sequence is null)\n" + usage);
    if (ignored) fprintf(stderr, "check-results: --config, -v, --quiet, -T and --threads have no effect here\n");
    dh_dazz *dt = nullptr, *dr = nullptr, *ds = nullptr;
    if (dh_dazz_open(pos[0].c_str(), &dt) || dh_dazz_open(pos[2].c_str(), &dr) || dh_dazz_open(pos[3].c_str(), &ds)) return fail(dh_last_error());
    const int32_t n_true = dh_dazz_nreads(dt), n_ref = dh_dazz_nreads(dr), n_res = dh_dazz_nreads(ds);
    const int64_t *toff = dh_dazz_offsets(dt), *qoff = dh_dazz_offsets(dr), *soff = dh_dazz_offsets(ds);
    // 2 crop < cutoff: the cutoff of the reference DB's stub, else its shortest contig
    long long cutoff = -1;
    {
        std::ifstream stub(pos[2]);
        std::string line;
        while (std::getline(stub, line)) {
            const size_t at = line.find("cutoff = ");
            if (at != std::string::npos) cutoff = atoll(line.c_str() + at + 9);
        }
        if (cutoff < 0)
            for (int32_t c = 0; c < n_ref; c++) cutoff = cutoff < 0 ? qoff[c + 1] - qoff[c] : std::min<long long>(cutoff, qoff[c + 1] - qoff[c]);
    }
    if (n_ref > 0 && (2 * crop >= cutoff || 2 * crop_amb >= cutoff))
        return fail("--crop-alignment and --crop-ambiguous: twice the crop must stay below the contig cutoff of " + std::to_string(cutoff));
    // ---- the mapped intervals are the input contigs, in order
    std::vector<int64_t> mptr, dptr;
    std::vector<int32_t> miv, div;
    std::string err = read_mask_track(dt, pos[0], pos[1], mptr, miv);
    if (!err.empty()) return fail(err);
    std::vector<int32_t> mapped;
    for (int32_t t = 0; t < n_true; t++)
        for (int64_t k = mptr[(size_t)t]; k < mptr[(size_t)t + 1]; k++) mapped.insert(mapped.end(), {t + 1, miv[(size_t)(2 * k)], miv[(size_t)(2 * k + 1)]});
    const int32_t n_input = (int32_t)(mapped.size() / 3);
    if (n_input != n_ref) return fail("the mask " + pos[1] + " has " + std::to_string(n_input) + " intervals, " + pos[2] + " has " + std::to_string(n_ref) + " contigs");
    bool have_dust = true;
    err = read_mask_track(dt, pos[0], dust_name, dptr, div);
    if (!err.empty()) {
        if (dust_given) return fail(err);
        have_dust = false;  // (the default track is used when it is there)
    }
    std::vector<int32_t> result_gap((size_t)n_res + 1, 0);
    for (int32_t c = 0; c + 1 < n_res; c++)
        if (dh_dazz_origin(ds)[c + 1] > dh_dazz_origin(ds)[c] && strcmp(dh_dazz_header(ds, c), dh_dazz_header(ds, c + 1)) == 0)
            result_gap[(size_t)c] = dh_dazz_fpulse(ds)[c + 1] - (int32_t)(dh_dazz_fpulse(ds)[c] + (soff[c + 1] - soff[c]));
    dh_ctx *ctx = nullptr;
    if (dh_ctx_create(0, nullptr, &ctx)) return fail(dh_last_error());
    // ---- findReferenceContigs: duplicates by the self search at --crop-ambiguous, mappings by the search in the result
    auto cropped = [&](long long by, std::vector<uint8_t> &b, std::vector<int64_t> &o) {
        o.assign(1, 0);
        for (int32_t c = 0; c < n_ref; c++) {
            const int64_t len = qoff[c + 1] - qoff[c];
            if (len > 2 * by) b.insert(b.end(), dh_dazz_bases(dr) + qoff[c] + by, dh_dazz_bases(dr) + qoff[c + 1] - by);
            o.push_back((int64_t)b.size());
        }
    };
    std::vector<uint8_t> qb;
    std::vector<int64_t> qo;
    std::vector<char> dup((size_t)n_ref + 1, 0);
    dh_exact_hits *hits = nullptr;
    cropped(crop_amb, qb, qo);
    if (dh_exact_locate(ctx, dh_dazz_bases(dr), qoff, n_ref, qb.data(), qo.data(), n_ref, 1, &hits)) return fail(dh_last_error());
    for (int64_t k = 0; k < dh_exact_hits_count(hits); k++) {
        const dh_exact_hit &h = dh_exact_hits_records(hits)[k];
        if (h.ref != h.query && qo[(size_t)h.query + 1] > qo[(size_t)h.query]) dup[(size_t)h.query] = 1;
    }
    dh_exact_hits_destroy(hits);
    qb.clear();
    cropped(crop, qb, qo);
    if (dh_exact_locate(ctx, dh_dazz_bases(ds), soff, n_res, qb.data(), qo.data(), n_ref, 1, &hits)) return fail(dh_last_error());
    std::vector<dh_contig_mapping> maps;
    for (int64_t k = 0; k < dh_exact_hits_count(hits); k++) {
        const dh_exact_hit &h = dh_exact_hits_records(hits)[k];
        if (qo[(size_t)h.query + 1] == qo[(size_t)h.query]) continue;  // (a contig the crop leaves empty is not searched)
        maps.push_back(dh_contig_mapping{h.ref + 1, (int32_t)h.begin, (int32_t)h.end, (int32_t)(soff[h.ref + 1] - soff[h.ref]), h.query + 1,
                                         dup[(size_t)h.query], h.complement, 0.0f});
    }
    dh_exact_hits_destroy(hits);
    // ---- the gaps
    dh_db *T = nullptr, *S = nullptr;
    if (dh_db_create(ctx, dh_dazz_bases(dt), toff, n_true, nullptr, &T) || dh_db_create(ctx, dh_dazz_bases(ds), soff, n_res, nullptr, &S))
        return fail(dh_last_error());
    dh_gap_report *rep = nullptr;
    if (dh_check_gaps(ctx, T, S, mapped.data(), n_input, maps.data(), (int32_t)maps.size(), result_gap.data(), have_dust ? dptr.data() : nullptr,
                      have_dust ? div.data() : nullptr, (int32_t)crop, nullptr, 1, n_input, &rep))
        return fail(dh_last_error());
    const dh_gap_summary *gs = dh_gap_report_summaries(rep);
    const dh_edit_paths *paths = dh_gap_report_paths(rep);
    auto ratio = [](double a, double b) { return b > 0 ? a / b : std::nan(""); };
    auto num = [](double x) {  // (NaN has no JSON text: null)
        char buf[40];
        snprintf(buf, sizeof(buf), "%.17g", x);
        return std::isnan(x) ? std::string("null") : std::string(buf);
    };
    static const char *const state_name[6] = {"unkown", "broken", "unclosed", "partiallyClosed", "closed", "ignored"};
    // ---- --gap-details: one object per gap that is not ignored (writeGapDetailsJson :1203-1239)
    if (!details.empty()) {
        FILE *f = fopen(details.c_str(), "w");
        if (!f) return fail("cannot write " + details);
        for (int32_t g = 0; g < n_input; g++) {
            const dh_gap_summary &s = gs[g];
            if (s.state == DH_GAP_IGNORED) continue;
            fprintf(f, "{\"leftContig\":%d,\"rightContig\":%d,\"state\":\"%s\",\"gapLength\":%d,\"details\":", g + 1, g + 2, state_name[s.state], s.gap_length);
            if (s.state == DH_GAP_CLOSED || s.state == DH_GAP_PARTIALLY_CLOSED) {
                std::string l[3];
                if (s.align_status == DH_CG_OK) {
                    const uint8_t *ops = dh_edit_paths_ops(paths) + dh_edit_paths_op_off(paths)[g];
                    const uint8_t *rb = dh_dazz_bases(dt) + toff[s.true_contig - 1] + s.true_begin;
                    // the query as the aligner saw it
                    std::vector<uint8_t> q;
                    const uint8_t *sb = dh_dazz_bases(ds);
                    if (s.result_begin_contig == s.result_end_contig)
                        q.assign(sb + soff[s.result_begin_contig - 1] + s.result_begin, sb + soff[s.result_begin_contig - 1] + s.result_end);
                    else {
                        q.assign(sb + soff[s.result_begin_contig - 1] + s.result_begin, sb + soff[s.result_begin_contig]);
                        q.insert(q.end(), (size_t)result_gap[(size_t)s.result_begin_contig - 1], (uint8_t)4);
                        q.insert(q.end(), sb + soff[s.result_end_contig - 1], sb + soff[s.result_end_contig - 1] + s.result_end);
                    }
                    if (s.complement) {
                        std::reverse(q.begin(), q.end());
                        for (auto &b : q) b = b < 4 ? (uint8_t)(3 - b) : b;
                    }
                    int64_t i = 0, j = 0;
                    for (int32_t k = 0; k < s.col_end; k++) {
                        const uint8_t op = ops[k];
                        const char rc_ = op == 2 ? '-' : "acgtn"[std::min<int>(rb[i++], 4)], qc = op == 1 ? '-' : "acgtn"[std::min<int>(q[(size_t)j++], 4)];
                        if (k < s.col_begin) continue;
                        l[0] += rc_, l[1] += op == 0 ? '|' : (op == 3 ? '.' : '-'), l[2] += qc;
                    }
                }
                // (cropReference does not carry the complement over: false at crop > 0, as in the reference)
                fprintf(f, "{\"referenceLength\":%d,\"queryLength\":%d,\"complement\":%s,\"percentIdentity\":%s,\"dustPercentIdentity\":%s,"
                           "\"noneDustPercentIdentity\":%s,\"alignment\":[\"%s\",\"%s\",\"%s\"]}",
                        s.reference_length, s.query_length, s.complement && crop == 0 ? "true" : "false", num(ratio(s.matches, s.col_end - s.col_begin)).c_str(),
                        num(ratio(s.dust_matches, s.dust_ops)).c_str(), num(ratio(s.none_dust_matches, s.none_dust_ops)).c_str(), l[0].c_str(), l[1].c_str(),
                        l[2].c_str());
            } else
                fprintf(f, "null");
            fprintf(f, ",\"sequence\":null}\n");
        }
        fclose(f);
    }
    // ---- the stats
    const unsigned long long none = ~0ull;
    unsigned long long bps_expected = 0, bps_known = 0, bps_result = (unsigned long long)soff[n_res], bps_gaps = 0;
    std::vector<unsigned long long> scaffolds, inputs, results, gap_len, closed_len;
    for (int32_t c = 0; c < n_input; c++) {
        const unsigned long long len = (unsigned long long)(mapped[3 * (size_t)c + 2] - mapped[3 * (size_t)c + 1]);
        bps_known += len, inputs.push_back(len);
        if (c == 0 || mapped[3 * (size_t)c] != mapped[3 * (size_t)c - 3]) scaffolds.push_back(0);
        int32_t first = c;
        while (first > 0 && mapped[3 * (size_t)first - 3] == mapped[3 * (size_t)c]) first--;
        scaffolds.back() = (unsigned long long)(mapped[3 * (size_t)c + 2] - mapped[3 * (size_t)first + 1]);
    }
    for (unsigned long long x : scaffolds) bps_expected += x;
    for (int32_t c = 0; c < n_res; c++) results.push_back((unsigned long long)(soff[c + 1] - soff[c]));
    double weighted = 0;
    long long correct = 0, closed = 0, partially = 0;
    for (int32_t g = 0; g < n_input; g++) {
        const dh_gap_summary &s = gs[g];
        if (s.state == DH_GAP_IGNORED) continue;
        const double identity = ratio(s.matches, s.col_end - s.col_begin);
        bps_gaps += (unsigned long long)s.gap_length, gap_len.push_back((unsigned long long)s.gap_length);
        weighted += identity * s.gap_length;
        partially += s.state == DH_GAP_PARTIALLY_CLOSED;
        if (s.state == DH_GAP_CLOSED) closed++, closed_len.push_back((unsigned long long)s.gap_length), correct += 1.0 <= identity;
    }
    std::vector<int32_t> per_contig((size_t)n_input + 1, 0);
    for (const dh_contig_mapping &m : maps) per_contig[(size_t)m.query_contig] += !m.duplicate;
    const long long mapped_contigs = std::count(per_contig.begin(), per_contig.end(), 1);
    auto n50 = [&](std::vector<unsigned long long> v) -> unsigned long long {  // util/math.d N!50 against numBpsExpected
        std::sort(v.begin(), v.end());
        double cum = 0;
        for (size_t k = v.size(); k-- > 0;)
            if ((cum += (double)v[k]) >= 0.5 * (double)bps_expected) return v[k];
        return 0;
    };
    auto median = [&](std::vector<unsigned long long> v) -> unsigned long long {
        if (v.empty()) return none;
        std::sort(v.begin(), v.end());
        return v.size() > 1 && v.size() % 2 == 0 ? (v[v.size() / 2 - 1] + v[v.size() / 2]) / 2 : v[v.size() / 2];
    };
    const double avg_err = bps_gaps ? weighted / (double)bps_gaps : std::nan("");
    const std::pair<const char *, unsigned long long> rows[] = {
        {"numContigsExpected", (unsigned long long)n_input}, {"numMappedContigs", (unsigned long long)mapped_contigs},
        {"numClosedGaps", (unsigned long long)closed}, {"numPartiallyClosedGaps", (unsigned long long)partially},
        {"numCorrectGaps", (unsigned long long)correct}, {"numBpsExpected", bps_expected}, {"numBpsKnown", bps_known},
        {"numBpsResult", bps_result}, {"numBpsInGaps", bps_gaps}, {"maximumN50", n50(scaffolds)}, {"inputN50", n50(inputs)},
        {"resultN50", n50(results)}, {"gapMedian", median(gap_len)}, {"closedGapMedian", median(closed_len)},
        {"minClosedGap", closed_len.empty() ? none : *std::min_element(closed_len.begin(), closed_len.end())},
        {"maxClosedGap", closed_len.empty() ? none : *std::max_element(closed_len.begin(), closed_len.end())}};
    if (json) {
        printf("{");
        for (const auto &r : rows) printf("\"%s\":%llu,", r.first, r.second);
        printf("\"averageInsertionError\":%s}\n", num(avg_err).c_str());
    } else {
        for (const auto &r : rows) printf("%-24s%20llu\n", (std::string(r.first) + ":").c_str(), r.second);
        printf("%-24s%20.3e\n", "averageInsertionError:", avg_err);
    }
    dh_gap_report_destroy(rep);
    dh_db_destroy(T);
    dh_db_destroy(S);
    dh_ctx_destroy(ctx);
    dh_dazz_close(dt), dh_dazz_close(dr), dh_dazz_close(ds);
    return 0;
}

int main(int argc, char **argv)
{
    g_tool = argv[0];
    const size_t slash = g_tool.find_last_of('/');
    if (slash != std::string::npos) g_tool = g_tool.substr(slash + 1);
    int first = 1;
    if (argc > 2 && std::string(argv[1]) == "--tool") {
        g_tool = argv[2];
        first = 3;
    }
    std::vector<std::string> args(argv + first, argv + argc);
    if (g_tool == "fasta2DB") return tool_fasta2(false, args);
    if (g_tool == "fasta2DAM") return tool_fasta2(true, args);
    if (g_tool == "DBsplit") return tool_dbsplit(args);
    if (g_tool == "DBrm") return tool_dbrm(args);
    if (g_tool == "DBdump") return tool_dbdump(args);
    if (g_tool == "DBshow") return tool_dbshow(args);
    if (g_tool == "DBdust") return tool_dbdust(args);
    if (g_tool == "LAmerge") return tool_lamerge(args);
    if (g_tool == "DAScover") return tool_qv("qual", args, false);
    if (g_tool == "DASqv") return tool_qv("qual", args, true);
    if (g_tool == "computeintrinsicqv") return tool_qv("inqual", args, true);
    if (g_tool == "daccord") return tool_daccord(args);
    if (g_tool == "merge-insertions") return tool_merge_insertions(args);
    if (g_tool == "LAsplit") return tool_lasplit(args);
    if (g_tool == "Catrack") return tool_catrack(args);
    if (g_tool == "TANmask") return tool_tanmask(args);
    if (g_tool == "LApaf") return tool_lapaf(args);
    if (g_tool == "LAtranspose") return tool_latranspose(args);
    if (g_tool == "DBnw") return tool_dbnw(args);
    if (g_tool == "stretcher") return tool_stretcher(args);
    if (g_tool == "fm-index") return tool_fm_index(args);
    if (g_tool == "chain-local-alignments") return tool_chain(args);
    if (g_tool == "propagate-mask") return tool_propagate_mask(args);
    if (g_tool == "validate-regions") return tool_validate_regions(args);
    if (g_tool == "collect") return tool_collect(args);
    if (g_tool == "mask-repetitive-regions") return tool_mask_repetitive_regions(args);
    if (g_tool == "merge-masks") return tool_merge_masks(args);
    if (g_tool == "filter-mask") return tool_filter_mask(args);
    if (g_tool == "check-results") return tool_check_results(args);
    die("unknown tool (expected fasta2DB fasta2DAM DBsplit DBrm DBdump DBshow DBdust LAmerge DAScover DASqv "
        "computeintrinsicqv daccord merge-insertions LAsplit Catrack TANmask LApaf LAtranspose DBnw stretcher fm-index "
        "chain-local-alignments propagate-mask validate-regions collect mask-repetitive-regions merge-masks filter-mask check-results)");
    return 1;
}
