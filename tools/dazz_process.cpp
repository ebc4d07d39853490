// dazz_process.cpp -- `dentist process` / `dentist process-pile-ups` and `dentist show-pile-ups` as an executable of its own
// (tools/process, copied under the other two names; the tool is chosen by argv[0] or `--tool <name>`).  The tools themselves
// are in dazz_dentist.cpp with DENTIST's other sub-commands; like tools/output they stay out of the table of dazz_main.cpp,
// which stays as the recorded command-line replay knows it.
#include "dazz_tools.h"

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
    if (g_tool == "process" || g_tool == "process-pile-ups") {
        g_tool = "process";  // (one tool under two names: its messages name it the same way)
        return tool_process(args);
    }
    if (g_tool == "show-pile-ups") return tool_show_pile_ups(args);
    die("unknown tool (expected process process-pile-ups show-pile-ups)");
}
