// option_table.cpp -- prints the generator's option table (drstencil_amd/csrc/generator.hpp: kOptions), one row per line: the
// spelling, then "hidden" for a row that help_text() leaves out.  Checked against the help text by tests/test_cli_and_ir.py.
#include <cstdio>
#include "generator.hpp"

int main() {
    for (const drs::Opt &r : drs::kOptions) std::printf("%s%s\n", r.name, (r.attr & drs::HIDDEN) ? " hidden" : "");
    return 0;
}
