// dazz_main.cpp -- the rest of the executable boundary of DENTIST's hot path over libdentist_hip.so: one multi-call binary,
// the tool is chosen by argv[0] (or `--tool <name>` as first argument) from the table below.  The tools live by role in
// dazz_db.cpp (DBs and their tracks), dazz_las.cpp (.las files and piles), dazz_align.cpp (base-level alignments, exact
// matches), dazz_dentist.cpp (DENTIST's own sub-commands) and dazz_check.cpp (check-results); each is described above its
// function, the helpers they share are in cli.h and dazz_tools.h.
// DENTIST only sees exit codes, files and stdout of these tools; flags it never emits are rejected.
#include "dazz_tools.h"

namespace {
struct Tool {
    const char *name;
    int (*run)(const Args &);
};
// (the names, in this order, are DAZZ_TOOLS of the Makefile, which copies the binary under each)
const Tool kTools[] = {
    {"fasta2DB", [](const Args &a) { return tool_fasta2(false, a); }},
    {"fasta2DAM", [](const Args &a) { return tool_fasta2(true, a); }},
    {"DBsplit", tool_dbsplit},
    {"DBrm", tool_dbrm},
    {"DBdump", tool_dbdump},
    {"DBshow", tool_dbshow},
    {"DBdust", tool_dbdust},
    {"LAmerge", tool_lamerge},
    {"DAScover", [](const Args &a) { return tool_qv("qual", a, false); }},
    {"DASqv", [](const Args &a) { return tool_qv("qual", a, true); }},
    {"computeintrinsicqv", [](const Args &a) { return tool_qv("inqual", a, true); }},
    {"daccord", tool_daccord},
    {"merge-insertions", tool_merge_insertions},
    {"LAsplit", tool_lasplit},
    {"Catrack", tool_catrack},
    {"TANmask", tool_tanmask},
    {"LApaf", tool_lapaf},
    {"LAtranspose", tool_latranspose},
    {"DBnw", tool_dbnw},
    {"stretcher", tool_stretcher},
    {"fm-index", tool_fm_index},
    {"chain-local-alignments", tool_chain},
    {"propagate-mask", tool_propagate_mask},
    {"validate-regions", tool_validate_regions},
    {"collect", tool_collect},
    {"mask-repetitive-regions", tool_mask_repetitive_regions},
    {"merge-masks", tool_merge_masks},
    {"filter-mask", tool_filter_mask},
    {"check-results", tool_check_results},
};
}  // namespace

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
    const Args args(argv + first, argv + argc);
    std::string names;
    for (const Tool &t : kTools) {
        if (g_tool == t.name) return t.run(args);
        names += std::string(names.empty() ? "" : " ") + t.name;
    }
    die("unknown tool (expected " + names + ")");
}
