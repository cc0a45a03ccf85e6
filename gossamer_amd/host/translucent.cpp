// translucent -- the `translucent trim-relative` / `translucent merge-graph-with-reference` executable
// (translucent.cc, TranslucentApp.cc): goss's driver under another name and table.
#include "GossHost.hpp"

#include <cstdio>
#include <cstdlib>
#include <unistd.h>

int main(int argc, char* argv[])
{
    const int rc = gosshost::translucentMain(argc, argv);
    // as goss ends (goss.cpp): the files are closed, the device runtime's tear-down is left to the kernel unless a tool
    // that writes from an exit handler is loaded with the process
    const char* full = std::getenv("GOSS_FULL_EXIT");
    if ((full && *full == '1') || std::getenv("LD_PRELOAD") || std::getenv("ROCP_TOOL_LIBRARIES") || std::getenv("ROCPROFILER_REGISTER_FORCE_LOAD"))
    {
        gosshost::releaseKeptBuffers();
        return rc;
    }
    std::fflush(nullptr);
    _exit(rc);
}
