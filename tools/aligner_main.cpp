// aligner_main.cpp -- drop-in `daligner` / `damapper` / `datander` executables over libdentist_hip.so.
//
// DENTIST spawns these tools by name with cwd = output directory and absolute (or stub) DB
// arguments and then expects `<A>.<B>.las` next to it (source/dentist/dazzler.d:6121-6170,
// getLasFile :4339-4354; literal instance tests/test-commands.sh:190-197).  The flag subset DENTIST
// emits is parsed (source/dentist/commandline.d:2886-2955); -m<track> loads the
// mask files DENTIST writes (dazzler.d:4870-5170) and excludes masked k-mers from seeding.  The mode is chosen
// by argv[0] (daligner | damapper | datander) or `--mode`.
#include <cmath>

#include "cli.h"  // (g_tool stays empty: the messages of this binary carry no prefix but the mode they name themselves)

struct OpenDb {
    Dazz dz;
    Db dev;
    std::string name;  // root[.block] as used in .las file names
};

static std::string las_name_part(const std::string &arg)
{
    std::string s = arg;
    const size_t slash = s.find_last_of('/');
    if (slash != std::string::npos) s = s.substr(slash + 1);
    for (const char *e : {".dam", ".db"}) {
        const size_t n = strlen(e);
        if (s.size() > n && s.compare(s.size() - n, n, e) == 0) s.resize(s.size() - n);
    }
    return s;
}

// union of the -m tracks that exist for this DB (a missing track is reported and skipped, the
// way daligner treats a track that was never computed for a block)
static void apply_masks(const std::string &arg, OpenDb &o, const std::vector<std::string> &tracks)
{
    std::vector<std::vector<std::pair<int32_t, int32_t>>> per((size_t)dh_dazz_nreads(o.dz.get()));
    bool any = false;
    for (const std::string &t : tracks) {
        std::vector<int64_t> ptr;
        std::vector<int32_t> iv;
        if (!read_mask(o.dz.get(), arg, t, ptr, iv).empty()) {
            fprintf(stderr, "mask track `%s` not found for %s: skipped\n", t.c_str(), arg.c_str());
            continue;
        }
        for (size_t i = 0; i < per.size(); i++)
            for (int64_t j = ptr[i]; j < ptr[i + 1]; j++) per[i].push_back({iv[(size_t)(2 * j)], iv[(size_t)(2 * j + 1)]});
        any = true;
    }
    if (!any) return;
    std::vector<int64_t> ptr;
    std::vector<int32_t> iv;
    merge_intervals(per, ptr, iv);
    iv.push_back(0);  // (never an empty array)
    CHK(dh_db_set_mask(o.dev.get(), ptr.data(), iv.data()));
}

static OpenDb open_db(dh_ctx *ctx, const std::string &arg, const std::vector<std::string> &tracks)
{
    OpenDb o;
    o.name = las_name_part(arg);
    o.dz = open_dazz(arg);
    CHK(dh_db_create(ctx, dh_dazz_bases(o.dz.get()), dh_dazz_offsets(o.dz.get()), dh_dazz_nreads(o.dz.get()), nullptr, into(o.dev)));
    if (!tracks.empty()) apply_masks(arg, o, tracks);
    return o;
}

// write one .las: ids are trimmed DB ids (block first id + local index)
static void write_las(const std::string &path, const dh_la_set *set, int afirst, int bfirst, int tspace)
{
    const int64_t n = dh_la_set_count(set);
    // chains that damapper's -n rule discards come back DISABLED: they are not written
    std::vector<dh_la> las;
    las.reserve((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        dh_la l = dh_la_set_records(set)[i];
        if (l.flags & DH_FLAG_DISABLED) continue;
        l.aread += afirst;
        l.bread += bfirst;
        las.push_back(l);
    }
    CHK(dh_las_write(path.c_str(), las.data(), (int64_t)las.size(), dh_la_set_trace(set), tspace));
}

int main(int argc, char **argv)
{
    std::string mode = argv[0];
    const size_t slash = mode.find_last_of('/');
    if (slash != std::string::npos) mode = mode.substr(slash + 1);
    dh_align_opts o;
    dh_default_align_opts(&o);
    bool flagA = false, flagI = false, flagC = false, verbose = false, seen_k = false, seen_w = false;
    double e = 0.7, near_best = 1.0;  // damapper's own -n default is 1.00 (best chains only); DENTIST always passes -n.7
    std::vector<std::string> dbs, tracks;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--mode" && i + 1 < argc) {
            mode = argv[++i];
            continue;
        }
        if (a.size() < 2 || a[0] != '-') {
            dbs.push_back(a);
            continue;
        }
        const char *v = a.c_str() + 2;
        switch (a[1]) {
        case 'k': o.k = atoi(v); seen_k = true; break;
        case 'w': o.band_shift = atoi(v); seen_w = true; break;
        case 'h': o.hmin = atoi(v); break;
        case 't': o.tcap = atoi(v); break;
        case 's': o.tspace = atoi(v); break;
        case 'l': o.min_len = atoi(v); break;
        case 'e': e = atof(v); break;
        case '%': o.kmer_mod = atoi(v); break;
        case 'A': flagA = true; break;
        case 'I': flagI = true; break;
        case 'C': flagC = true; break;
        case 'v': verbose = true; break;
        case 'm': tracks.push_back(v); break;
        case 'T': case 'P': case 'M': break;  // threads / temp dir / memory: no meaning on the device
        case 'n': near_best = atof(v); break;
        case 'B': case 'b': case 'p': case 'z': case 'H':
            // accepted for DENTIST's argv, but not implemented: say so instead of silently differing
            fprintf(stderr, "%s: option %s is accepted but has no effect in this implementation\n", mode.c_str(), a.c_str());
            break;
        default: die(mode + ": unknown option " + a);
        }
    }
    if (mode.find("datander") != std::string::npos) {
        if (dbs.empty()) die("usage: datander [-v] [-k<int(12)>] [-w<int(4)>] [-h<int(35)>] [-T<int(4)>] [-P<dir>] [-e<double(.70)>] [-l<int(500)>] [-s<int(100)>] <path:db|dam> ...");
    } else if (dbs.size() < 2)
        die("usage: " + mode + " [-k -w -h -t -s -l -e -A -I -C -T -m...] <subject:db|dam> <target:db|dam> ...");
    if (e <= 0.5 || e >= 1.0) die(mode + ": -e must be in (0.5, 1)");
    o.pen = (int)floor(2.0 / (1.0 - e));
    o.max_err_ppm = (int)llround((1.0 - e) * 1e6);
    const bool mapper = mode.find("damapper") != std::string::npos;
    const bool tander = mode.find("datander") != std::string::npos;
    if (mapper && o.min_len == 500 && o.tspace == 100) o.min_len = 500;
    if (mapper) {
        // damapper: the tiled band extension (one alignment per lane) and chains with the -n near-best rule
        o.algo = 1;
        o.width = 64;
        if (near_best < 0 || near_best > 1) die(mode + ": -n must be in [0, 1]");
    }

    Ctx ctx;
    CHK(dh_ctx_create(0, nullptr, into(ctx)));
    if (tander) {
        // datander <block> ...: every read of a block against ITSELF, the local alignments off the main diagonal (tandem
        // repeats) -> TAN.<block>.las (DAMASKER; DENTIST's call: `datander -T<n> -s126 -l500 -e0.7 <dam>.<block>`,
        // commandline.d:2866-2876, snakemake/Snakefile:1056-1076; TANmask reads the file).  Its own defaults: -k12 -w4 -h35.
        if (!seen_k) o.k = 12;
        if (!seen_w) o.band_shift = 4;
        o.algo = 1;
        o.width = 64;
        o.strands = 1;
        o.skip_self = 3;
        for (const std::string &arg : dbs) {
            const OpenDb A = open_db(ctx.get(), arg, tracks);
            const int first = dh_dazz_first_id(A.dz.get());
            LaSet set;
            CHK(dh_align_db(ctx.get(), A.dev.get(), A.dev.get(), &o, 0, into(set)));
            write_las("TAN." + A.name + ".las", set.get(), first, first, o.tspace);
            if (verbose) fprintf(stderr, "datander: %lld local alignments -> TAN.%s.las\n", (long long)dh_la_set_count(set.get()), A.name.c_str());
        }
        return 0;
    }
    if (mapper) CHK(dh_ctx_set_near_best(ctx.get(), (int32_t)llround(near_best * 1e6)));
    const OpenDb A = open_db(ctx.get(), dbs[0], tracks);
    const int afirst = dh_dazz_first_id(A.dz.get());
    for (size_t bi = 1; bi < dbs.size(); bi++) {
        const bool same = las_name_part(dbs[bi]) == A.name;
        OpenDb other;
        if (!same) other = open_db(ctx.get(), dbs[bi], tracks);
        const OpenDb &B = same ? A : other;
        const int bfirst = dh_dazz_first_id(B.dz.get());
        dh_align_opts oo = o;
        // one DB against itself: every unordered pair once, both records written (daligner's own
        // behaviour); -I also aligns a read against itself, which needs the plain all-vs-all
        oo.skip_self = (same && !flagI) ? 2 : 0;
        if (oo.skip_self == 2) {
            oo.max_la = std::max(oo.max_la, 64);
            oo.max_cand = std::max(oo.max_cand, 128);
        }
        LaSet ab, ba;
        // damapper -C, and daligner on two DBs without -A (which writes A.B.las and B.A.las, dazzler.d:6121-6140; the
        // workflow's block pairs `daligner -I ... ref.i ref.j`, Snakefile:998-1022): the second file comes out of the same
        // pass -- the transposed pair of every alignment, through its seed (dh_align_db_transposed; DH-2, the tiled band)
        const bool both = !same && !mapper && !flagA;
        if (both) {
            oo.algo = 1;
            oo.width = 64;
        }
        const bool transposed = !same && ((mapper && flagC) || both);
        if (transposed)
            CHK(dh_align_db_transposed(ctx.get(), A.dev.get(), B.dev.get(), &oo, mapper ? 1 : 0, into(ab), into(ba)));
        else
            CHK(dh_align_db(ctx.get(), A.dev.get(), B.dev.get(), &oo, mapper ? 1 : 0, into(ab)));
        write_las(A.name + "." + B.name + ".las", ab.get(), afirst, bfirst, o.tspace);
        if (verbose) fprintf(stderr, "%s: %lld local alignments -> %s.%s.las\n", mode.c_str(), (long long)dh_la_set_count(ab.get()), A.name.c_str(), B.name.c_str());
        if (ba) write_las(B.name + "." + A.name + ".las", ba.get(), bfirst, afirst, o.tspace);
    }
    return 0;
}
