// dazz_tools.h -- the tools of the multi-call binary, one function each (dazz_main.cpp picks it by name), and what their
// translation units share beyond cli.h.
#pragma once
#include "cli.h"

using Args = std::vector<std::string>;

// dazz_db.cpp: building, showing and masking a DAZZ_DB
int tool_fasta2(bool dam, const Args &args);
int tool_dbsplit(const Args &args);
int tool_dbrm(const Args &args);
int tool_dbdump(const Args &args);
int tool_dbshow(const Args &args);
int tool_dbdust(const Args &args);
int tool_catrack(const Args &args);
// dazz_las.cpp: .las files and what is computed from their piles
int tool_lamerge(const Args &args);
int tool_lasplit(const Args &args);
int tool_tanmask(const Args &args);
int tool_qv(const char *track, const Args &args, bool write);
int tool_daccord(const Args &args);
int tool_merge_insertions(const Args &args);
// dazz_align.cpp: base-level alignments and exact matches
int tool_lapaf(const Args &args);
int tool_latranspose(const Args &args);
int tool_dbnw(const Args &args);
int tool_stretcher(const Args &args);
int tool_fm_index(const Args &args);
// dazz_dentist.cpp: DENTIST's own sub-commands
int tool_chain(const Args &args);
int tool_propagate_mask(const Args &args);
int tool_validate_regions(const Args &args);
int tool_collect(const Args &args);
int tool_mask_repetitive_regions(const Args &args);
int tool_merge_masks(const Args &args);
int tool_filter_mask(const Args &args);
int tool_process(const Args &args);        // (these two are reached through tools/process, whose main is in dazz_process.cpp)
int tool_show_pile_ups(const Args &args);
// dazz_check.cpp
int tool_check_results(const Args &args);
// dazz_output.cpp: `output`, an executable of its own (its main is there)
int tool_output(const Args &args);

std::string slurp(FILE *f);
inline char base_char(uint8_t b) { return "acgtn"[std::min<int>(b, 4)]; }
inline std::string with_las_suffix(std::string p) { return p.size() < 4 || p.compare(p.size() - 4, 4, ".las") != 0 ? p + ".las" : p; }

// dir/root.ext of a DB path and the files of its tracks (dazz_db.cpp)
struct DbPath {
    std::string dir, root, ext;  // dir/root.ext (ext "db" or "dam"), block > 0 when the path names one
    int32_t block = 0;
    std::string block_db(int32_t b) const { return dir + "/" + root + (b > 0 ? "." + std::to_string(b) : "") + "." + ext; }
};
DbPath parse_db_path(std::string p);
int32_t stub_blocks(const DbPath &d);
std::string track_file(const DbPath &d, int32_t block, const std::string &name, const char *ext);
void write_mask_files(const DbPath &d, int32_t block, const std::string &name, int32_t nreads, const std::vector<int64_t> &ptr,
                      const std::vector<int32_t> &iv);

// Mask track `name` of the whole DB `da`; `<block>.<mask>` names the track of that block (dazz_dentist.cpp).  "" or what failed.
std::string read_mask_track(const dh_dazz *da, const std::string &db_path, const std::string &name, std::vector<int64_t> &ptr,
                            std::vector<int32_t> &iv);
