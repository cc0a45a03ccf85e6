// xenome -- the `xenome index` / `xenome classify` executable (xenome.cc, XenoApp.cc): goss's driver under another
// name and table.
#include "GossHost.hpp"

int main(int argc, char* argv[])
{
    gosshost::runAndExit(gosshost::xenomeMain, argc, argv);
}
