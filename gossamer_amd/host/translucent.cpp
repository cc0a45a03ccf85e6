// translucent -- the `translucent trim-relative` / `translucent merge-graph-with-reference` executable
// (translucent.cc, TranslucentApp.cc): goss's driver under another name and table.
#include "GossHost.hpp"

int main(int argc, char* argv[])
{
    gosshost::runAndExit(gosshost::translucentMain, argc, argv);
}
