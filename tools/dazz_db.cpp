// dazz_db.cpp -- the tools that build, show and mask a DAZZ_DB, and the paths of a DB's files.
#include <cctype>
#include <cmath>

#include "dazz_tools.h"

std::string slurp(FILE *f)
{
    std::string s;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, got);
    return s;
}
static bool is_dam(const std::string &p) { return p.size() > 4 && p.compare(p.size() - 4, 4, ".dam") == 0; }

// fasta2DB / fasta2DAM  -i <db>  (FASTA on stdin) | <db> <fasta>...   dazzler.d:6233-6330
int tool_fasta2(bool dam, const Args &args)
{
    bool from_stdin = false;
    Args pos;
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

// DBsplit [-f] [-a] [-x<n>] [-s<mb>] <db>   dazzler.d:6332-6345
int tool_dbsplit(const Args &args)
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

// DBrm <db>...   dazzler.d:6115-6119
int tool_dbrm(const Args &args)
{
    for (const std::string &a : args)
        if (a[0] != '-') CHK(dh_dazz_remove(a.c_str()));
    return 0;
}

// record numbers (1-based) from `ids` / `a-b` arguments; empty = all
static std::vector<int32_t> record_list(const Args &sel, int32_t first, int32_t n)
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

// DBdump [-r -h -s -i] <db> [ids | a-b]   SURVEY Appendix B grammar   dazzler.d:6445-6505, parser :2788-3078
int tool_dbdump(const Args &args)
{
    bool fr = false, fh = false, fs = false, fi = false;
    std::string db;
    Args sel;
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
    const Dazz dz = open_dazz(db);
    const dh_dazz *d = dz.get();
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
            for (int64_t x = 0; x < l; x++) seq[(size_t)x] = base_char(bases[off[i] + x]);
            printf("S %lld %s\n", (long long)l, seq.c_str());
        }
        if (fi) {
            const int64_t a = qptr[(size_t)i], b = qptr[(size_t)i + 1];
            std::string q;
            for (int64_t x = a; x < b; x++) q.push_back(qv_char(qv[(size_t)x]));
            printf("I %lld %s\n", (long long)(b - a), q.c_str());
        }
    }
    return 0;
}

// DBshow [-n] <db> [ids]   FASTA / scaffold structure lines   dazzler.d:4609-4690, 6507-6517
int tool_dbshow(const Args &args)
{
    bool names = false;
    int width = 80;
    std::string db;
    Args sel;
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
    const Dazz dz = open_dazz(db);
    const dh_dazz *d = dz.get();
    const int32_t n = dh_dazz_nreads(d), first = dh_dazz_first_id(d);
    const std::vector<int32_t> ids = record_list(sel, first, n);
    const int64_t *off = dh_dazz_offsets(d);
    const uint8_t *bases = dh_dazz_bases(d);
    const bool dam = is_dam(db) || (n > 0 && dh_dazz_header(d, 0)[0] == '>');
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
            for (int64_t y = x; y < e; y++) putchar(base_char(bases[off[i] + y]));
            putchar('\n');
        }
    }
    return 0;
}

// DBdust <db>   writes the `dust` mask track   processPileUps/package.d:476, 655
int tool_dbdust(const Args &args)
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
    const Dev v(db);
    CHK(dh_db_dust(v.db.get()));
    const int32_t n = dh_dazz_nreads(v.dz.get());
    std::vector<int64_t> ptr((size_t)n + 1);
    const int64_t m = dh_db_get_mask(v.db.get(), ptr.data(), nullptr, 0);
    if (m < 0) die(dh_last_error());
    std::vector<int32_t> iv((size_t)std::max<int64_t>(2 * m, 2));
    dh_db_get_mask(v.db.get(), ptr.data(), iv.data(), m);
    CHK(dh_dazz_write_mask(db.c_str(), "dust", n, ptr.data(), iv.data()));
    return 0;
}

// ---------------------------------------------------------------------------------- the files of a DB and its tracks
DbPath parse_db_path(std::string p)
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
int32_t stub_blocks(const DbPath &d)
{
    FILE *f = fopen(d.block_db(0).c_str(), "r");
    if (!f) die("cannot open the DB stub");
    char line[512];
    int32_t nb = 0;
    while (fgets(line, sizeof(line), f))
        if (sscanf(line, "blocks = %d", &nb) == 1) break;
    fclose(f);
    return nb;
}
std::string track_file(const DbPath &d, int32_t block, const std::string &name, const char *ext)
{
    return d.dir + "/." + d.root + (block > 0 ? "." + std::to_string(block) : "") + "." + name + "." + ext;
}
void write_mask_files(const DbPath &d, int32_t block, const std::string &name, int32_t nreads, const std::vector<int64_t> &ptr,
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

// Catrack [-v] [-f] [-d] <db> <track>: the block mask tracks .<db>.<block>.<track>.{anno,data} concatenated into the DB's
// track (snakemake/Snakefile:1111-1123; track layout dazzler.d:4943-5170)
int tool_catrack(const Args &args)
{
    Args pos;
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
