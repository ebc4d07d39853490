// dazz_las.cpp -- the tools over .las files: merging and splitting them, and what is computed from the piles of a read (tandem
// mask, intrinsic QVs, consensus); merge-insertions is here as the other file-merging helper of the workflow.
#include "dazz_tools.h"

// LAmerge <out.las> <in.las>...   snakemake/Snakefile:1173-1185
int tool_lamerge(const Args &args)
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
    out = with_las_suffix(out);
    CHK(dh_las_merge(in.data(), (int32_t)in.size(), out.c_str()));
    return 0;
}

// LAsplit <target with @ or #> <parts> < <source.las>: the workflow's split of a merged .las for the validation blocks
// (snakemake/Snakefile:1426-1434).  The records of the .las on stdin in <parts> files of nearly equal size; a file ends only
// where the A read changes (the piles of an A read stay together: every consumer of a block file reads piles).  '@' or '#'
// in the target is the part number, 1-based.
int tool_lasplit(const Args &args)
{
    Args pos;
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
    const std::string tmp = with_las_suffix(std::string(pos[0]).replace(mark, 1, "stdin-tmp"));
    {
        const std::string raw = slurp(stdin);
        FILE *f = fopen(tmp.c_str(), "wb");
        if (!f || fwrite(raw.data(), 1, raw.size(), f) != raw.size() || fclose(f) != 0) die("cannot write " + tmp);
    }
    LaSet set;
    const int rc = dh_las_read(tmp.c_str(), into(set));
    remove(tmp.c_str());
    if (rc) die(std::string("dh_las_read: ") + dh_last_error());
    const int64_t n = dh_la_set_count(set.get());
    const dh_la *la = dh_la_set_records(set.get());
    const uint16_t *tr = dh_la_set_trace(set.get());
    const int32_t ts = dh_la_set_tspace(set.get());
    int64_t at = 0;
    for (int32_t k = 1; k <= parts; k++) {
        int64_t end = k == parts ? n : std::min<int64_t>(n, (n * k + parts - 1) / parts);
        end = std::max(end, at);
        while (end > at && end < n && la[end].aread == la[end - 1].aread) end++;  // do not cut a pile
        const std::string out = with_las_suffix(std::string(pos[0]).replace(mark, 1, std::to_string(k)));
        // (records keep their trace offsets into the whole trace array)
        CHK(dh_las_write(out.c_str(), la + at, end - at, tr, ts));
        at = end;
    }
    return 0;
}

// TANmask [-v] [-l<int(500)>] [-n<track(tan)>] <db> <TAN las>...   (snakemake/Snakefile:1095-1108)
// A local alignment of a read with itself (datander) marks a tandem repeat -- the union of its A and B intervals, when at
// least -l long, goes into the mask; intervals of a read are merged.  One track per .las: the block's when the file name
// carries a block number (TAN.<db>.<block>.las), the DB's otherwise.
int tool_tanmask(const Args &args)
{
    Args pos;
    int32_t minlen = 500;
    std::string name = "tan", v;
    for (const std::string &a : args) {
        if (a == "-v") continue;
        if (short_value(a, 'l', &v))
            minlen = atoi(v.c_str());
        else if (short_value(a, 'n', &name))
            ;
        else if (a[0] == '-')
            die("unknown option " + a);
        else
            pos.push_back(a);
    }
    if (pos.size() < 2) die("usage: TANmask [-v] [-l<int(500)>] [-n<track(tan)>] <subject:db|dam> <overlaps:las> ...");
    const DbPath d = parse_db_path(pos[0]);
    for (size_t f = 1; f < pos.size(); f++) {
        const std::string lp = with_las_suffix(pos[f]);
        // block of the file: "<...>.<root>.<block>.las"
        int32_t block = 0;
        {
            const std::string stem = lp.substr(0, lp.size() - 4);
            const size_t dot = stem.find_last_of('.');
            if (dot != std::string::npos && dot + 1 < stem.size() && stem.find_first_not_of("0123456789", dot + 1) == std::string::npos)
                block = atoi(stem.c_str() + dot + 1);
        }
        const Dazz db = open_dazz(d.block_db(block));
        const int32_t n = dh_dazz_nreads(db.get()), first = dh_dazz_first_id(db.get());
        dh_la_set *set = nullptr;
        CHK(dh_las_read(lp.c_str(), &set));  // (spelled as the message quotes it)
        const LaSet owner(set);
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
        std::vector<int64_t> ptr;
        std::vector<int32_t> iv;
        merge_intervals(per, ptr, iv);
        write_mask_files(d, block, name, n, ptr, iv);
    }
    return 0;
}

// DAScover -v <db> <las> ; DASqv -v -c<cov> <db> <las>: the `qual` track (dazzler.d:6142-6156);
// computeintrinsicqv -d<depth> <db> <las>: the `inqual` track (dazzler.d:6172-6183).
// The intrinsic QV per trace tile of every read as a byte track; the overlaps are those of a pile-up DB.
int tool_qv(const char *track, const Args &args, bool write)
{
    int cov = 0;
    Args pos;
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
    const Dev v(pos[0]);
    const int32_t n = dh_dazz_nreads(v.dz.get()), first = dh_dazz_first_id(v.dz.get());
    const LaSet set = read_las(pos[1]);
    const std::vector<dh_la> las = shifted_records(set.get(), first, first);
    const int32_t ts = dh_la_set_tspace(set.get());
    if (cov <= 0) cov = std::max(4, n);
    const int64_t *off = dh_dazz_offsets(v.dz.get());
    int32_t maxtiles = 1;
    for (int32_t i = 0; i < n; i++) maxtiles = std::max<int32_t>(maxtiles, (int32_t)((off[i + 1] - off[i] + ts - 1) / ts));
    std::vector<uint8_t> qv((size_t)n * maxtiles, 255);
    CHK(dh_tile_qv(v.ctx, v.db.get(), las.data(), (int64_t)las.size(), dh_la_set_trace(set.get()), ts, cov, qv.data(), maxtiles));
    std::vector<int64_t> ptr((size_t)n + 1, 0);
    std::vector<uint8_t> data;
    for (int32_t i = 0; i < n; i++) {
        const int32_t nt = (int32_t)((off[i + 1] - off[i] + ts - 1) / ts);
        for (int32_t t = 0; t < nt; t++) data.push_back(std::min<uint8_t>(qv[(size_t)i * maxtiles + t], 50));
        ptr[(size_t)i + 1] = (int64_t)data.size();
    }
    data.push_back(0);
    CHK(dh_dazz_write_track(pos[0].c_str(), track, n, ptr.data(), data.data()));
    return 0;
}

// daccord [-t<n>] [-I<i>,<j>] [-f] [--eprofonly] <las> <db>   dazzler.d:6185-6231
// consensus FASTA on stdout; --eprofonly writes <las>.eprof
int tool_daccord(const Args &args)
{
    int i0 = -1, i1 = -1, rounds = 3;
    bool eprof_only = false;
    Args pos;
    for (const std::string &a : args) {
        if (a.compare(0, 2, "-I") == 0) {
            if (sscanf(a.c_str() + 2, "%d,%d", &i0, &i1) != 2) die("bad -I");
        } else if (a == "--eprofonly")
            eprof_only = true;
        else if (a == "-f" || a.compare(0, 2, "-t") == 0 || a.compare(0, 2, "-w") == 0 || a.compare(0, 2, "-a") == 0 ||
                 a.compare(0, 2, "-k") == 0 || a.compare(0, 2, "-m") == 0 || a.compare(0, 2, "-d") == 0 || a.compare(0, 2, "-V") == 0)
            ;
        else if (a.compare(0, strlen("--rounds="), "--rounds=") == 0)
            rounds = atoi(a.c_str() + strlen("--rounds="));
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
    const Dev v(pos[1]);
    const int32_t n = dh_dazz_nreads(v.dz.get()), first = dh_dazz_first_id(v.dz.get());
    const LaSet set = read_las(pos[0]);
    const std::vector<dh_la> las = shifted_records(set.get(), first, first);
    if (i0 < 0) {
        i0 = 0;
        i1 = n - 1;
    }
    if (i0 > i1 || i1 >= n) die("-I outside the DB");
    const int64_t *off = dh_dazz_offsets(v.dz.get());
    for (int32_t r = i0; r <= i1; r++) {
        std::vector<uint8_t> cns((size_t)(off[r + 1] - off[r]) * 6 + 64);
        int64_t len = 0;
        CHK(dh_consensus(v.ctx, v.db.get(), las.data(), (int64_t)las.size(), dh_la_set_trace(set.get()), dh_la_set_tspace(set.get()), r, rounds,
                         cns.data(), (int64_t)cns.size(), &len));
        // header in daccord's style: read id (0-based) / segment / 0_length
        printf(">%d/0/0_%lld A=[0,%lld]\n", r, (long long)len, (long long)len);
        for (int64_t x = 0; x < len; x += 80) {
            for (int64_t y = x; y < std::min(len, x + 80); y++) putchar(base_char(cns[(size_t)y]));
            putchar('\n');
        }
    }
    return 0;
}

// merge-insertions <merged.db> <batch.db>...: DENTIST's own sub-command (commands/mergeInsertions.d:42-164,
// snakemake/Snakefile:1315-1334), here so that batches written by this library can be merged without the D binary
int tool_merge_insertions(const Args &args)
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
