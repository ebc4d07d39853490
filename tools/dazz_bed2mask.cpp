// dazz_bed2mask.cpp -- `dentist bed2mask` as an executable of its own (tools/bed2mask): like tools/output and tools/process it
// stays out of the table of dazz_main.cpp, which stays as the recorded command-line replay knows it.  Host only: no device is
// asked for and no context is created.
//
// bed2mask [--bed=<file>] [--data-comments] <ref-db> <out-mask>
// The intervals of a BED file (standard input without --bed) in scaffold coordinates written as the mask <out-mask> of the
// contigs of <ref-db> (dh_bed_to_mask: commands/bed2mask.d:70-333; snakemake/Snakefile:1437-1466).  With --data-comments column 4
// (`contigs-<a>-<b>|reads-<id>-...`, what `output --closed-gaps-bed` writes) is stored with the mask as two track extras, in
// this order: `contigs`, two ids per interval, and `reads`, per interval the count and then the ids -- both int64 and exact.
// An unknown option prints the usage and exits 1; everything else that fails exits 2 with the library's message.
#include "cli.h"

using BedMask = Handle<dh_bed_mask, dh_bed_mask_destroy>;

static std::string slurp_all(FILE *f)
{
    std::string s;
    char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, got);
    return s;
}

int main(int argc, char **argv)
{
    g_tool = "bed2mask";
    const char *usage = "usage: bed2mask [--bed=<file>] [--data-comments] [--config=<file>] [-v] [--quiet] [-T<n>] <ref-db> <out-mask>";
    std::vector<std::string> pos;
    std::string bed_file;
    bool ignored = false, data_comments = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (long_value(a, "--bed=", &bed_file))
            continue;
        if (a == "--data-comments")
            data_comments = true;
        else if (ignored_option(a))
            ignored = true;
        else if (is_option(a))
            die("unknown or malformed option " + a + "\n" + usage);
        else
            pos.push_back(a);
    }
    if (pos.size() != 2) die(usage);
    if (ignored) notice_ignored();
    Dazz da;
    must(dh_dazz_open(pos[0].c_str(), into(da)));
    std::string text;
    if (bed_file.empty())
        text = slurp_all(stdin);
    else {
        FILE *f = fopen(bed_file.c_str(), "rb");
        if (!f) fail("cannot open " + bed_file);
        text = slurp_all(f);
        fclose(f);
    }
    BedMask m;
    must(dh_bed_to_mask(da.get(), text.data(), (int64_t)text.size(), bed_file.empty() ? "-" : bed_file.c_str(), data_comments ? 1 : 0, into(m)));
    const int64_t count = dh_bed_mask_count(m.get());
    must(write_mask(pos[0], pos[1], dh_bed_mask_ncontigs(m.get()), dh_bed_mask_ptr(m.get()), dh_bed_mask_iv(m.get()), count));
    if (data_comments) {  // writeDazzlerMask, bed2mask.d:314-331
        must(dh_dazz_write_extra(pos[0].c_str(), pos[1].c_str(), "contigs", DH_EXTRA_INT64, DH_ACCUM_EXACT, dh_bed_mask_contig_ids(m.get()), 2 * count));
        const int64_t *off = dh_bed_mask_read_off(m.get()), *ids = dh_bed_mask_read_ids(m.get());
        std::vector<int64_t> reads;
        for (int64_t i = 0; i < count; i++) {
            reads.push_back(off[i + 1] - off[i]);
            reads.insert(reads.end(), ids + off[i], ids + off[i + 1]);
        }
        reads.push_back(0);  // (never an empty array)
        must(dh_dazz_write_extra(pos[0].c_str(), pos[1].c_str(), "reads", DH_EXTRA_INT64, DH_ACCUM_EXACT, reads.data(), (int64_t)reads.size() - 1));
    }
    return 0;
}
