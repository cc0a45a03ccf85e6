// electus -- the `electus index` / `electus classify` executable (electus.cc, ElectApp.cc): goss's driver under another
// name and table.
#include "GossHost.hpp"

int main(int argc, char* argv[])
{
    gosshost::runAndExit(gosshost::electusMain, argc, argv);
}
