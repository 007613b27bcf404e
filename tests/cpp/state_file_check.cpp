// state_file_check.cpp -- the state file's parser (pi-slam-fusion_amd/csrc/state_file.hpp, the very code the library compiles) on files
// a test wrote: built with -fsanitize=address,undefined by tests/test_state_file.py and run on good and hostile files alike.  One line
// per file, in the order given:
//   ok <map type> <pyramid type> <bands> <weight type> <tiles> <w> <h> <version> <bounds that were not finite>
//   refused <reason>
// and, for a file that is accepted, every slot image is read through read_slot (as load_state reads it) and summed into the line.
// Exit status 0 whatever the files hold: a sanitizer report is what fails the run.
#include "state_file.hpp"

#include <cstdio>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
    namespace sf = pf::statefile;
    for (int i = 1; i < argc; i++) {
        sf::StateHeader h;
        std::vector<sf::TileHead> heads;
        std::string why;
        std::FILE* f = std::fopen(argv[i], "rb");
        if (!f) { std::printf("refused cannot open\n"); continue; }
        if (!sf::scan(f, h, &heads, why)) { std::printf("refused %s\n", why.c_str()); std::fclose(f); continue; }
        // the raw heads once more: how many bounds did sanitize() replace?
        long replaced = 0;
        unsigned long long sum = 0;
        std::vector<unsigned char> slot((size_t)h.slot_bytes);
        bool ok = true;
        for (size_t k = 0; ok && k < heads.size(); k++) {
            sf::TileHead raw;
            ok = fseeko(f, (off_t)(sizeof(sf::StateHeader) + k * sf::record_bytes(h)), SEEK_SET) == 0 && std::fread(&raw, sizeof(raw), 1, f) == 1;
            for (int c = 0; ok && c < 16; c++) replaced += std::memcmp(&raw.wlb[c], &heads[k].wlb[c], 4) != 0;
            ok = ok && sf::read_slot(f, h, k, slot.data());
            for (unsigned char b : slot) sum += b;
        }
        std::fclose(f);
        if (!ok) { std::printf("refused cannot read a record that was scanned\n"); continue; }
        std::printf("ok %d %d %d %d %llu %d %d %u %ld sum %llu\n", h.map_type, h.pyramid_type, h.band_number, h.weight_type, (unsigned long long)h.n_tiles, h.w, h.h,
                    h.version, replaced, sum);
    }
    return 0;
}
