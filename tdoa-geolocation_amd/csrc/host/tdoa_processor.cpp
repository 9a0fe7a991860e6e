// tdoa_processor -- host harness over the C ABI (include/tdoa_mi355x.h) that keeps the
// reference processor's command line and file conventions (processor.go:1047-1075):
//
//   tdoa_processor [options] <ref_freq_hz> <target_freq_hz> <csv_file> <dat_file1> <dat_file2> <dat_file3> ...
//
// Same inputs: lat-lon-table.csv (Name,Latitude,Longitude,Elevation; the reference
// transmitter is the row named "%.0f" of <ref_freq_hz>, processor.go:59-99), raw .dat
// captures named after their station (substring match, processor.go:110-122), three equal
// blocks [f1 | f2 | f1] (processor.go:211-233).  Same flow: pairs i<j, reference blocks then
// target blocks, delay -> seconds -> metres, 3-station solve on the target differences.
// Default mode calls the drop-in tdoa_cross_correlate_c64 (the reference's executed chain);
// --fm runs the batched north-star path (u8 -> FM discriminator -> FFT xcorr -> peak).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/tdoa_mi355x.h"

namespace {

struct Station {
    std::string name;
    double lat = 0, lon = 0, elev = 0;
};

struct Capture {
    Station st;
    std::string path;
    std::vector<uint8_t> raw;
};

const double kC = 299792458.0;   // processor.go:873

std::string basename_of(const std::string &p)
{
    size_t s = p.find_last_of('/');
    return s == std::string::npos ? p : p.substr(s + 1);
}

// processor.go:52-107 loadStations
bool load_stations(const std::string &csv, std::vector<Station> *out, std::string *err)
{
    std::ifstream f(csv);
    if (!f) { *err = "failed to open CSV file: " + csv; return false; }
    std::string line;
    bool header = true;
    while (std::getline(f, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        if (header) { header = false; continue; }          // Name,Latitude,Longitude,Elevation
        std::stringstream ss(line);
        std::string name, a, b, c;
        if (!std::getline(ss, name, ',') || !std::getline(ss, a, ',') || !std::getline(ss, b, ',') || !std::getline(ss, c, ','))
            continue;                                         // short rows are skipped like the reference
        Station s;
        s.name = name;
        char *e1, *e2, *e3;
        s.lat = std::strtod(a.c_str(), &e1);
        s.lon = std::strtod(b.c_str(), &e2);
        s.elev = std::strtod(c.c_str(), &e3);
        if (e1 == a.c_str() || e2 == b.c_str() || e3 == c.c_str()) { *err = "invalid number in CSV row: " + line; return false; }
        out->push_back(s);
    }
    return true;
}

// >1 GiB safe whole-file read (a single os.File.Read silently stops at 1 GiB in the reference)
bool read_file(const std::string &path, std::vector<uint8_t> *out, std::string *err)
{
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { *err = "failed to open file: " + path; return false; }
    if (std::fseek(f, 0, SEEK_END) != 0) { std::fclose(f); *err = "failed to get file size: " + path; return false; }
    const long long size = std::ftell(f);                     // -1 on a directory, FIFO or other unseekable path
    if (size < 0 || std::fseek(f, 0, SEEK_SET) != 0) { std::fclose(f); *err = "failed to get file size: " + path; return false; }
    out->resize((size_t)size);
    size_t got = 0;
    while (got < (size_t)size) {
        size_t n = std::fread(out->data() + got, 1, std::min<size_t>((size_t)size - got, 1u << 28), f);
        if (n == 0) break;
        got += n;
    }
    std::fclose(f);
    if (got != (size_t)size) { *err = "failed to read data: " + path; return false; }
    return true;
}

void usage(const char *argv0)
{
    std::printf("Usage: %s [--fm] [--fine] [--stack[=WINDOWS]] [--drift=H[/D]] [--track=J] [--closure=G[/SEP]] [--locate=ROWSxCOLS/SPAN_KM] [--locate-track=J[/SEP]] [--emitters=K[/GUARD]] [--zoom-emitters] [--track-emitters=K[/GUARD]] [--map-stats=R1[,R2...][/FOOT]] [--locate-upsample=U] [--locate-zoom=Z[/H[/SEP]]] [--locate-track-zoom=Z[/H[/JF[/SEP]]]] [--sync=LAT,LON,HEIGHT[/G[/R]]] [--sync-drift=H[/D]] [--sync-drift-fine=U[/RF]] [--sync-fine=U[/RF]] [--one-call] [--gate SAMPLES] [--device N] [--window SAMPLES] [--max-lag SAMPLES] [--k1-smooth SAMPLES] [--k1-gate] "
                "<ref_freq_hz> <target_freq_hz> <csv_file> <dat_file1> [dat_file2] [dat_file3] ...\n", argv0);
    std::printf("Example: %s 162400000 101700000 lat-lon-table.csv kx0u-data.dat n3pay-data.dat kf0mtl-data.dat\n", argv0);
}

// the stacks tdoa_num_stacks counted for --stack=WINDOWS on blocks of wpb windows: the windows of a full stack and of stack
// sid (the last stack of a block may be short)
struct Stacks {
    int wpb = 0, m = 0, spb = 0, n = 0;
    Stacks() {}
    Stacks(int wpb_, int stack_m, int spb_, int n_) : wpb(wpb_), m(stack_m > 0 && stack_m < wpb_ ? stack_m : wpb_), spb(spb_), n(n_) {}
    int n_w(int sid) const { return std::min(m, wpb - (sid % spb) * m); }
};

double median(std::vector<double> v)
{
    if (v.empty()) return 0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

}  // namespace

int main(int argc, char **argv)
{
    bool fm = false, fine = false, stack = false;
    int stack_m = 0;         // --stack=WINDOWS: windows per stack (0, or plain --stack: a whole block)
    bool drift = false;      // --drift=H[/D] (with --stack): stack along the best of the slopes -H/D .. H/D lags per window
    int drift_h = 0, drift_d = 1;
    bool track = false;      // --track=J (with --stack): one lag per window of every stack, at most J lags apart (tdoa_process_track)
    int track_j = 0;
    bool closure = false;    // --closure=G[/SEP] (with --stack): per stack and station triple the three lags that close (tdoa_process_closure)
    int closure_g = 0, closure_sep = 1;
    // --locate=ROWSxCOLS/SPAN_KM (with --stack): per stack the best cell of a square grid of that span centred on the stations'
    // centroid, at their mean height (tdoa_process_locate)
    bool locate = false;
    int locate_rows = 0, locate_cols = 0;
    double locate_km = 0.0;
    // --sync=LAT,LON,HEIGHT[/G[/R]] (with --stack --locate, whole-block stacks): the reference emitter's position; the stations'
    // clocks are searched on the two reference blocks within G samples, R sweeps (tdoa_process_sync), and the locate runs with
    // them -- blocks 1 and 3 with their own clocks, block 2 with their midpoint (tdoa_locate_set_clock)
    // --locate-track=J[/SEP] (with --stack --locate): per block the best track of cells through its stacks' maps, consecutive
    // cells at most J rows and columns apart (tdoa_process_locate_track)
    bool locate_track = false;
    int ltrack_j = 0, ltrack_sep = 1;
    // --emitters=K[/GUARD] (with --stack --locate): per stack K fixes, each searched with the lags within GUARD of the earlier
    // fixes' lags counting 0 in every pair (tdoa_process_locate_multi)
    bool emitters = false;
    int emitters_k = 1, emitters_guard = 2;
    // --zoom-emitters (with --emitters and --locate-zoom): the rounds and every round's window of the fine grid in one call
    // (tdoa_process_locate_multi_zoom); an EMITTER-ZOOM line per round behind the LOCATE-MULTI lines, which keep their bytes
    bool zoom_emitters = false;
    // --track-emitters=K[/GUARD] (with --stack --locate --locate-track): per block K tracks, each tracked with the lags within
    // GUARD of the earlier tracks' lags counting 0 in every stack's pairs (tdoa_process_locate_track_multi)
    bool track_emitters = false;
    int temitters_k = 1, temitters_guard = 2;
    // --map-stats=R1[,R2...][/FOOT] (with --stack --locate): a STATS line after every LOCATE, LOCATE-MULTI and track line -- the
    // judged plane's live cells, its words at ranks R / 65535 of them (32768: the median) and the cells that reach FOOT / 65536
    // of the way from the first of those words to the best (tdoa_locate_set_stats)
    bool map_stats = false;
    std::vector<uint16_t> stats_ranks;
    int stats_foot = 0;
    // --locate-upsample=U (with --stack --locate), U in 2, 4, 8, 16: the searches score their cells on the surfaces upsampled to
    // 1/U sample (tdoa_locate_set_upsample); a grid finer than one lag of range difference needs it
    int locate_up = 1;
    // --locate-zoom=Z[/H[/SEP]] (with --stack --locate): every stack's best cell is searched again on the (2H+1)^2 cells around it of
    // the same grid at Z cells per cell, ((ROWS-1) Z + 1) x ((COLS-1) Z + 1) cells, in the same call (tdoa_process_locate_zoom); a
    // ZOOM line follows every LOCATE line.  H defaults to 2 Z, SEP to 1
    bool locate_zoom = false;
    int zoom_z = 1, zoom_h = -1, zoom_sep = 1;
    // --locate-track-zoom=Z[/H[/JF[/SEP]]] (with --stack --locate --locate-track): every block's track is followed again through the
    // (2H+1)^2-cell windows around its cells on the same grid at Z cells per cell, consecutive fine cells at most JF rows and
    // columns apart, in the same call (tdoa_process_locate_track_zoom); a TRACKZOOM line follows every block's LOCATE-TRACK lines.
    // H defaults to 2 Z, JF to Z (at most 16), SEP to 1
    bool track_zoom = false;
    int tzoom_z = 1, tzoom_h = -1, tzoom_jf = -1, tzoom_sep = 1;
    bool sync = false;
    double sync_lat = 0, sync_lon = 0, sync_h = 0;
    int sync_g = 128, sync_r = 2;
    // --sync-drift=H[/D] (with --sync; any --stack=M): the stations' clock offsets and rates, slopes up to H / D lags per stack, are
    // searched along each reference block's stacks (tdoa_process_sync_drift); blocks 1 and 3 are located under their own lines'
    // clocks, block 2 under block 1's line continued over its positions (tdoa_sync_line_clock)
    bool sync_drift = false;
    int sdrift_h = 0, sdrift_d = 1;
    // --sync-fine=U[/RF] (with --sync, whole-block stacks), U in 2, 4, 8, 16: the clocks of --sync are refined to 1/U sample in RF
    // sweeps on the upsampled surfaces' words (tdoa_process_sync_fine); blocks 1 and 3 are located under their own refined clocks,
    // block 2 under the midpoint of the two rows rounded to 1/16 sample
    bool sync_fine = false;
    // --one-call (with --stack --locate --sync --sync-fine --locate-zoom): the clocks, the target block's midpoint row and the zoom
    // locate in one call (tdoa_process_sync_locate): the clocks stay on the device and the stacks are accumulated once.  Prints
    // what the run without the flag prints.  Also with --stack=M --locate --sync --sync-drift --sync-drift-fine --locate-track
    // --locate-track-zoom: the fine lines, the target block's rows (block 1's fine line continued) and the zoomed tracks in one call
    // (tdoa_process_sync_drift_locate); the same stdout at --sync-drift-fine=16
    bool one_call = false;
    int sfine_u = 16, sfine_r = 2;
    // --sync-drift-fine=U[/RF] (with --sync-drift), U in 2, 4, 8, 16: the lines' offsets and rates are refined to 1/U sample in RF
    // sweeps (tdoa_process_sync_drift_fine); blocks 1 and 3 are located under their own fine rows, block 2 under block 1's fine
    // line continued over its positions (tdoa_sync_line_clock16)
    bool sync_drift_fine = false;
    int sdfine_u = 16, sdfine_r = 2;
    double gate = 120.0;     // samples; PROJECT_NOTES.md:29-32 (max |TDOA| about 57 us = 114 samples at 2 Msps)
    tdoa_params prm;
    tdoa_default_params(&prm);
    std::vector<std::string> pos;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a == "--fm") fm = true;
        else if (a == "--fine") fm = fine = true;              // sub-sample refinement + plausibility gate (implies --fm)
        else if (a == "--stack") fm = stack = true;            // one delay per block and pair from the summed surfaces (implies --fm)
        else if (a.rfind("--stack=", 0) == 0) { fm = stack = true; stack_m = std::atoi(a.c_str() + 8); }
        else if (a.rfind("--drift=", 0) == 0) {
            drift = true;
            drift_h = std::atoi(a.c_str() + 8);
            const size_t slash = a.find('/');
            drift_d = slash == std::string::npos ? 1 : std::atoi(a.c_str() + slash + 1);
        }
        else if (a.rfind("--track=", 0) == 0) { track = true; track_j = std::atoi(a.c_str() + 8); }
        else if (a.rfind("--closure=", 0) == 0) {
            closure = true;
            closure_g = std::atoi(a.c_str() + 10);
            const size_t slash = a.find('/');
            closure_sep = slash == std::string::npos ? 1 : std::atoi(a.c_str() + slash + 1);
        }
        else if (a.rfind("--locate=", 0) == 0) {
            locate = true;
            if (std::sscanf(a.c_str() + 9, "%dx%d/%lf", &locate_rows, &locate_cols, &locate_km) != 3 || locate_rows < 1 || locate_cols < 1 ||
                (long long)locate_rows * locate_cols > (1ll << 22) || !(locate_km > 0.0)) {
                std::fprintf(stderr, "--locate=ROWSxCOLS/SPAN_KM with ROWS x COLS in 1 .. 2^22 and SPAN_KM > 0, e.g. --locate=64x64/40\n");
                return 1;
            }
        }
        else if (a.rfind("--locate-track=", 0) == 0) {
            locate_track = true;
            const int got = std::sscanf(a.c_str() + 15, "%d/%d", &ltrack_j, &ltrack_sep);
            if (got < 1 || ltrack_j < 0 || ltrack_j > 16 || ltrack_sep < 1) {
                std::fprintf(stderr, "--locate-track=J[/SEP] with J in 0 .. 16 and SEP >= 1, e.g. --locate-track=1\n");
                return 1;
            }
        }
        else if (a.rfind("--emitters=", 0) == 0) {
            emitters = true;
            const int got = std::sscanf(a.c_str() + 11, "%d/%d", &emitters_k, &emitters_guard);
            if (got < 1 || emitters_k < 1 || emitters_k > TDOA_LOCATE_MAX_EMITTERS || emitters_guard < 0) {
                std::fprintf(stderr, "--emitters=K[/GUARD] with K in 1 .. 8 and GUARD >= 0, e.g. --emitters=2/2\n");
                return 1;
            }
        }
        else if (a.rfind("--map-stats=", 0) == 0) {
            map_stats = true;
            const std::string arg = a.substr(12), list = arg.substr(0, arg.find('/'));
            bool ok = !list.empty();
            for (size_t at = 0; ok && at <= list.size();) {
                const size_t end = std::min(list.find(',', at), list.size());
                char *stop = nullptr;
                const long r = std::strtol(list.c_str() + at, &stop, 10);
                ok = end > at && stop == list.c_str() + end && r >= 0 && r <= 65535;
                stats_ranks.push_back((uint16_t)r);
                at = end + 1;
            }
            if (ok && arg.find('/') != std::string::npos) {
                char *stop = nullptr;
                const char *f = arg.c_str() + arg.find('/') + 1;
                const long v = std::strtol(f, &stop, 10);
                ok = *f && !*stop && v >= 0 && v <= 65535;
                stats_foot = (int)v;
            }
            if (!ok || stats_ranks.size() > TDOA_MAP_STATS_MAX_RANKS) {
                std::fprintf(stderr, "--map-stats=R1[,R2...][/FOOT] with 1 .. 8 ranks and FOOT in 0 .. 65535, e.g. --map-stats=32768,64880/49152\n");
                return 1;
            }
        }
        else if (a.rfind("--locate-upsample=", 0) == 0) {
            locate_up = std::atoi(a.c_str() + 18);
            if (locate_up != 1 && locate_up != 2 && locate_up != 4 && locate_up != 8 && locate_up != 16) {
                std::fprintf(stderr, "--locate-upsample=U with U one of 1, 2, 4, 8, 16, e.g. --locate-upsample=4\n");
                return 1;
            }
        }
        else if (a.rfind("--locate-zoom=", 0) == 0) {
            locate_zoom = true;
            const int got = std::sscanf(a.c_str() + 14, "%d/%d/%d", &zoom_z, &zoom_h, &zoom_sep);
            if (got < 2) zoom_h = zoom_z >= 1 && zoom_z <= 32 ? 2 * zoom_z : 64;
            if (got < 1 || zoom_z < 1 || zoom_z > 64 || zoom_h < 0 || zoom_h > 64 || zoom_sep < 1) {
                std::fprintf(stderr, "--locate-zoom=Z[/H[/SEP]] with Z in 1 .. 64, H in 0 .. 64 and SEP >= 1, e.g. --locate-zoom=8/16\n");
                return 1;
            }
        }
        else if (a.rfind("--locate-track-zoom=", 0) == 0) {
            track_zoom = true;
            const int got = std::sscanf(a.c_str() + 20, "%d/%d/%d/%d", &tzoom_z, &tzoom_h, &tzoom_jf, &tzoom_sep);
            if (got < 2) tzoom_h = tzoom_z >= 1 && tzoom_z <= 32 ? 2 * tzoom_z : 64;
            if (got < 3) tzoom_jf = tzoom_z >= 1 && tzoom_z <= 16 ? tzoom_z : 16;
            if (got < 1 || tzoom_z < 1 || tzoom_z > 64 || tzoom_h < 0 || tzoom_h > 64 || tzoom_jf < 0 || tzoom_jf > 16 || tzoom_sep < 1) {
                std::fprintf(stderr, "--locate-track-zoom=Z[/H[/JF[/SEP]]] with Z in 1 .. 64, H in 0 .. 64, JF in 0 .. 16 and SEP >= 1, e.g. "
                                     "--locate-track-zoom=8/16/8\n");
                return 1;
            }
        }
        else if (a == "--zoom-emitters")
            zoom_emitters = true;
        else if (a.rfind("--track-emitters=", 0) == 0) {
            track_emitters = true;
            const int got = std::sscanf(a.c_str() + 17, "%d/%d", &temitters_k, &temitters_guard);
            if (got < 1 || temitters_k < 1 || temitters_k > TDOA_LOCATE_MAX_EMITTERS || temitters_guard < 0) {
                std::fprintf(stderr, "--track-emitters=K[/GUARD] with K in 1 .. 8 and GUARD >= 0, e.g. --track-emitters=2/2\n");
                return 1;
            }
        }
        else if (a.rfind("--sync=", 0) == 0) {
            sync = true;
            const int got = std::sscanf(a.c_str() + 7, "%lf,%lf,%lf/%d/%d", &sync_lat, &sync_lon, &sync_h, &sync_g, &sync_r);
            if (got < 3 || sync_g < 0 || sync_g > 1023 || sync_r < 0 || sync_r > 16) {
                std::fprintf(stderr, "--sync=LAT,LON,HEIGHT[/G[/R]] with G in 0 .. 1023 and R in 0 .. 16, e.g. --sync=41.257,-95.955,349/128/2\n");
                return 1;
            }
        }
        else if (a.rfind("--sync-drift=", 0) == 0) {
            sync_drift = true;
            const int got = std::sscanf(a.c_str() + 13, "%d/%d", &sdrift_h, &sdrift_d);
            if (got < 1 || sdrift_h < 0 || sdrift_h > 512 || sdrift_d < 1) {
                std::fprintf(stderr, "--sync-drift=H[/D] with H in 0 .. 512 and D >= 1, e.g. --sync-drift=16/4\n");
                return 1;
            }
        }
        else if (a.rfind("--sync-drift-fine=", 0) == 0) {
            sync_drift_fine = true;
            const int got = std::sscanf(a.c_str() + 18, "%d/%d", &sdfine_u, &sdfine_r);
            if (got < 1 || (sdfine_u != 2 && sdfine_u != 4 && sdfine_u != 8 && sdfine_u != 16) || sdfine_r < 0 || sdfine_r > 16) {
                std::fprintf(stderr, "--sync-drift-fine=U[/RF] with U one of 2, 4, 8, 16 and RF in 0 .. 16, e.g. --sync-drift-fine=16/2\n");
                return 1;
            }
        }
        else if (a.rfind("--sync-fine=", 0) == 0) {
            sync_fine = true;
            const int got = std::sscanf(a.c_str() + 12, "%d/%d", &sfine_u, &sfine_r);
            if (got < 1 || (sfine_u != 2 && sfine_u != 4 && sfine_u != 8 && sfine_u != 16) || sfine_r < 0 || sfine_r > 16) {
                std::fprintf(stderr, "--sync-fine=U[/RF] with U one of 2, 4, 8, 16 and RF in 0 .. 16, e.g. --sync-fine=16/2\n");
                return 1;
            }
        }
        else if (a == "--one-call") one_call = true;
        else if (a == "--gate" && i + 1 < argc) gate = std::atof(argv[++i]);
        else if (a == "--device" && i + 1 < argc) prm.device = std::atoi(argv[++i]);
        else if (a == "--window" && i + 1 < argc) prm.window_len = std::atoll(argv[++i]);
        else if (a == "--max-lag" && i + 1 < argc) prm.max_lag = std::atoi(argv[++i]);
        else if (a == "--k1-smooth" && i + 1 < argc) prm.k1_smooth = std::atoi(argv[++i]);   // the prebuilt binary's chain uses 10
        else if (a == "--k1-gate") prm.k1_gate = 1;                                          // its power gate (envelope branch)
        else pos.push_back(a);
    }
    if (drift && !stack) { std::fprintf(stderr, "--drift needs --stack\n"); return 1; }
    if (track && !stack) { std::fprintf(stderr, "--track needs --stack\n"); return 1; }
    if (closure && !stack) { std::fprintf(stderr, "--closure needs --stack\n"); return 1; }
    if (locate && !stack) { std::fprintf(stderr, "--locate needs --stack\n"); return 1; }
    if (locate_track && !locate) { std::fprintf(stderr, "--locate-track needs --stack --locate\n"); return 1; }
    if (emitters && !locate) { std::fprintf(stderr, "--emitters needs --stack --locate\n"); return 1; }
    if (zoom_emitters && (!emitters || !locate_zoom)) {
        std::fprintf(stderr, "usage: --zoom-emitters needs --stack --locate=... --emitters=K[/GUARD] --locate-zoom=Z[/H[/SEP]]\n");
        return 1;
    }
    if (track_emitters && !locate_track) { std::fprintf(stderr, "--track-emitters needs --stack --locate --locate-track\n"); return 1; }
    if (map_stats && !locate) { std::fprintf(stderr, "--map-stats needs --stack --locate\n"); return 1; }
    if (locate_up != 1 && !locate) { std::fprintf(stderr, "--locate-upsample needs --stack --locate\n"); return 1; }
    if (locate_zoom && !locate) { std::fprintf(stderr, "--locate-zoom needs --stack --locate\n"); return 1; }
    if (locate_zoom && ((long long)(locate_rows - 1) * zoom_z + 1) * ((long long)(locate_cols - 1) * zoom_z + 1) > (1ll << 22)) {
        std::fprintf(stderr, "--locate-zoom: the fine grid of %lld x %lld cells has more than 2^22 cells\n", (long long)(locate_rows - 1) * zoom_z + 1,
                     (long long)(locate_cols - 1) * zoom_z + 1);
        return 1;
    }
    if (track_zoom && !locate_track) { std::fprintf(stderr, "--locate-track-zoom needs --stack --locate --locate-track\n"); return 1; }
    if (track_zoom && ((long long)(locate_rows - 1) * tzoom_z + 1) * ((long long)(locate_cols - 1) * tzoom_z + 1) > (1ll << 22)) {
        std::fprintf(stderr, "--locate-track-zoom: the fine grid of %lld x %lld cells has more than 2^22 cells\n",
                     (long long)(locate_rows - 1) * tzoom_z + 1, (long long)(locate_cols - 1) * tzoom_z + 1);
        return 1;
    }
    if (sync && !locate) { std::fprintf(stderr, "--sync needs --stack --locate\n"); return 1; }
    if (sync_drift && !sync) { std::fprintf(stderr, "--sync-drift needs --stack --locate --sync\n"); return 1; }
    if (sync_drift_fine && !sync_drift) { std::fprintf(stderr, "--sync-drift-fine needs --stack --locate --sync --sync-drift\n"); return 1; }
    if (sync_fine && (!sync || sync_drift)) { std::fprintf(stderr, "--sync-fine needs --stack --locate --sync and no --sync-drift\n"); return 1; }
    if (one_call && (!sync_fine || !locate_zoom) && (!sync_drift_fine || !track_zoom)) {
        std::fprintf(stderr, "--one-call needs --stack --locate --sync --sync-fine --locate-zoom\n");
        return 1;
    }
    if (sync && !sync_drift && stack_m != 0) { std::fprintf(stderr, "--sync needs whole-block stacks: --stack without =WINDOWS\n"); return 1; }
    if (pos.size() < 4) {                                     // processor.go:1048-1052
        usage(argv[0]);
        return 1;
    }
    char *end = nullptr;
    const double ref_freq = std::strtod(pos[0].c_str(), &end);
    if (end == pos[0].c_str()) { std::fprintf(stderr, "Invalid reference frequency: %s\n", pos[0].c_str()); return 1; }
    const double tgt_freq = std::strtod(pos[1].c_str(), &end);
    if (end == pos[1].c_str()) { std::fprintf(stderr, "Invalid target frequency: %s\n", pos[1].c_str()); return 1; }
    std::vector<Station> stations;
    std::string err;
    if (!load_stations(pos[2], &stations, &err)) { std::fprintf(stderr, "Failed to create processor: %s\n", err.c_str()); return 1; }
    char refname[64];
    std::snprintf(refname, sizeof(refname), "%.0f", ref_freq);          // processor.go:96
    const Station *ref = nullptr;
    for (auto &s : stations)
        if (s.name == refname) ref = &s;
    if (!ref) { std::fprintf(stderr, "Failed to create processor: reference frequency %s not found in stations\n", refname); return 1; }
    std::printf("Loaded %zu stations including reference %.0f MHz\n", stations.size(), ref_freq / 1e6);
    if (pos.size() - 3 < 3) {                                 // processor.go:740-742
        std::fprintf(stderr, "TDOA processing failed: need at least 3 collector stations, got %zu\n", pos.size() - 3);
        return 1;
    }
    std::printf("Processing TDOA for target frequency %.3f MHz\n", tgt_freq / 1e6);

    std::vector<Capture> caps;
    for (size_t i = 3; i < pos.size(); i++) {
        Capture c;
        c.path = pos[i];
        const std::string base = basename_of(pos[i]);
        bool found = false;
        for (auto &s : stations)
            if (base.find(s.name) != std::string::npos) { c.st = s; found = true; break; }
        if (!found) { std::fprintf(stderr, "TDOA processing failed: could not identify station from filename: %s\n", pos[i].c_str()); return 1; }
        size_t n_samples = 0;
        if (fm) {
            // the batched path streams the file straight to the GPU later: only its size is needed here
            FILE *f = std::fopen(pos[i].c_str(), "rb");
            if (!f) { std::fprintf(stderr, "TDOA processing failed: failed to open file: %s\n", pos[i].c_str()); return 1; }
            std::fseek(f, 0, SEEK_END);
            const long long size = std::ftell(f);
            std::fclose(f);
            if (size < 0) { std::fprintf(stderr, "TDOA processing failed: failed to get file size: %s\n", pos[i].c_str()); return 1; }
            n_samples = (size_t)size / 2;
        } else {
            if (!read_file(pos[i], &c.raw, &err)) { std::fprintf(stderr, "TDOA processing failed: %s\n", err.c_str()); return 1; }
            n_samples = c.raw.size() / 2;
        }
        std::printf("Loaded collector: %s at %.6f°, %.6f°, %.1fm (%zu samples)\n", c.st.name.c_str(), c.st.lat, c.st.lon,
                    c.st.elev, n_samples);
        caps.push_back(std::move(c));
    }
    const int S = (int)caps.size();

    std::printf("\nBaseline distances (3D):\n");                // processor.go:802-809
    for (int i = 0; i < S; i++)
        for (int j = i + 1; j < S; j++) {
            double a[3], b[3];
            tdoa_latlon_to_ecef(caps[i].st.lat, caps[i].st.lon, caps[i].st.elev, a);
            tdoa_latlon_to_ecef(caps[j].st.lat, caps[j].st.lon, caps[j].st.elev, b);
            const double d = std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
            std::printf("%s - %s: %.2f km\n", caps[i].st.name.c_str(), caps[j].st.name.c_str(), d / 1000);
        }

    tdoa_ctx *ctx = nullptr;
    int rc = tdoa_create(&prm, &ctx);
    if (rc != TDOA_OK) { std::fprintf(stderr, "tdoa_create: %s\n", tdoa_strerror(rc)); return 2; }
    auto die = [&](const char *what, int code) {
        std::fprintf(stderr, "%s: %s (%s)\n", what, tdoa_strerror(code), tdoa_last_error(ctx));
        tdoa_destroy(ctx);
        return 2;
    };

    std::vector<double> tgt_dt;                                // seconds, pairs i<j
    std::vector<double> tgt_w;
    if (!fm) {
        // ---- the reference's executed flow: complex64 signals, crossCorrelate per pair
        std::vector<std::vector<float>> refs(S), tgts(S);
        for (int s = 0; s < S; s++) {
            const size_t n = caps[s].raw.size() / 2;
            std::vector<float> data(2 * n);
            if ((rc = tdoa_load_iq_u8(ctx, caps[s].raw.data(), n, data.data()))) return die("tdoa_load_iq_u8", rc);
            const size_t bs = n / 3;                           // processor.go:214
            if (bs == 0) { refs[s] = data; tgts[s] = data; continue; }
            refs[s].assign(data.begin(), data.begin() + 2 * bs);                                   // block 1
            refs[s].insert(refs[s].end(), data.begin() + 4 * bs, data.begin() + 6 * bs);           // block 3
            tgts[s].assign(data.begin() + 2 * bs, data.begin() + 4 * bs);                          // block 2
            const size_t chunk = (size_t)prm.window_len;       // processor.go:772-780
            if (refs[s].size() / 2 > chunk) refs[s].resize(2 * chunk);
            if (tgts[s].size() / 2 > chunk) tgts[s].resize(2 * chunk);
        }
        for (int kind = 0; kind < 2; kind++) {
            std::printf(kind == 0 ? "\n=== REFERENCE SIGNAL CORRELATION TEST ===\n" : "\n=== TARGET SIGNAL CORRELATION TEST ===\n");
            auto &sig = kind == 0 ? refs : tgts;
            // one call for all pairs: every station's signal goes through preprocessSignal once instead of once per pair
            // (processor.go:629-630); the numbers are the per-pair crossCorrelate's, bit for bit
            std::vector<const float *> ptr(S);
            std::vector<size_t> len(S);
            for (int s = 0; s < S; s++) { ptr[s] = sig[s].data(); len[s] = sig[s].size() / 2; }
            std::vector<int32_t> delays((size_t)S * (S - 1) / 2);
            std::vector<double> corrs(delays.size());
            if ((rc = tdoa_cross_correlate_batch_c64(ctx, ptr.data(), len.data(), S, delays.data(), corrs.data())))
                return die("tdoa_cross_correlate_batch_c64", rc);
            int pidx = 0;
            for (int i = 0; i < S; i++)
                for (int j = i + 1; j < S; j++, pidx++) {
                    const int32_t delay = delays[pidx];
                    const double corr = corrs[pidx];
                    const double dt = (double)delay / prm.sample_rate;       // processor.go:821-822
                    std::printf("%s %s - %s: delay=%d samples (%.3f μs), correlation=%.17g\n", kind == 0 ? "REF" : "TGT",
                                caps[i].st.name.c_str(), caps[j].st.name.c_str(), delay, dt * 1e6, corr);
                    if (kind == 1) { tgt_dt.push_back(dt); tgt_w.push_back(std::fabs(corr)); }
                }
        }
    } else {
        // ---- north-star path: raw bytes in, one peak per (window, pair) out
        size_t shortest = (size_t)-1;            // samples of the shortest capture: a window is window_len of them, or a whole block
        for (int s = 0; s < S; s++) { // file -> pinned staging -> HBM
            size_t n_samples = 0;
            if ((rc = tdoa_capture_upload_file(ctx, s, caps[s].path.c_str(), &n_samples))) return die("tdoa_capture_upload_file", rc);
            shortest = std::min(shortest, n_samples);
        }
        const long long wlen = std::min<long long>(prm.window_len, (long long)(shortest / 3));
        int wpb = 0, W = 0;
        if ((rc = tdoa_num_windows(ctx, &wpb, &W))) return die("tdoa_num_windows", rc);
        const int P = tdoa_num_pairs(ctx);
        {
            // capture QA in the spirit of collector.go:204-248 (validateDataFile), on every window instead of 1000 samples:
            // mean block power per station, REF blocks consistent within 2x, TGT block different from REF by > 50 %
            std::vector<tdoa_window_quality> q((size_t)W * S);
            if ((rc = tdoa_window_quality_all(ctx, 0, 1, q.data()))) return die("tdoa_window_quality_all", rc);
            std::printf("\n=== CAPTURE QUALITY (mean power of (I-127.5)^2+(Q-127.5)^2 per block) ===\n");
            for (int s = 0; s < S; s++) {
                double pw[3] = {0, 0, 0};
                int clip = 0, overload = 0;
                for (int w = 0; w < W; w++) {
                    const tdoa_window_quality &x = q[(size_t)w * S + s];
                    pw[w / wpb] += x.mean_power / wpb;
                    clip += x.has_clipping;
                    overload += x.has_overload;
                }
                // an all-127/128 block has power 0.25 at least, but an empty or all-127.5-equivalent one must not print inf/NaN
                const auto ratio = [](double a, double b) { return b > 0 ? a / b : 0.0; };
                const double ref_ratio = ratio(pw[2], pw[0]);                       // collector.go:231
                const double tgt_ratio = (ratio(pw[1], pw[0]) + ratio(pw[1], pw[2])) / 2.0; // collector.go:240-242
                std::printf("%s: REF %.2f  TGT %.2f  REF %.2f  | REF blocks %s (%.2fx), TGT/REF %.2fx%s | %d clipped, %d low-level windows of %d\n",
                            caps[s].st.name.c_str(), pw[0], pw[1], pw[2],
                            (ref_ratio > 2.0 || ref_ratio < 0.5) ? "INCONSISTENT" : "consistent", ref_ratio, tgt_ratio,
                            (tgt_ratio > 1.5 || tgt_ratio < 0.67) ? "" : " (very similar)", clip, overload, W);
            }
        }
        std::vector<tdoa_peak> peaks((size_t)W * P);
        std::vector<tdoa_fine_peak> fines;
        if (fine) {
            fines.resize((size_t)W * P);
            if ((rc = tdoa_process_fine(ctx, 0, 1, gate, peaks.data(), fines.data()))) return die("tdoa_process_fine", rc);
        } else if ((rc = tdoa_process(ctx, 0, 1, peaks.data(), nullptr))) return die("tdoa_process", rc);
        // --stack: the windows' surfaces of a block added lag by lag (tdoa_process_stacked), two peaks per stack-pair
        int spb = 0, n_stacks = 0;
        Stacks stacks;
        std::vector<tdoa_peak> spk;
        std::vector<int32_t> scnt;
        std::vector<tdoa_fine_peak> sfine;
        std::vector<int32_t> sdrift;             // --drift: h* per stack-pair (tdoa_process_stacked_drift)
        std::vector<tdoa_peak> tscore;           // --track: the score and the lags of every stack-pair's track (tdoa_process_track)
        std::vector<int32_t> tlags;
        std::vector<tdoa_closure> clos;          // --closure: one record per stack and station triple (tdoa_process_closure)
        std::vector<tdoa_location> locs;         // --locate: one record per stack (tdoa_process_locate)
        std::vector<tdoa_zoom> zooms;            // --locate-zoom: one more record per stack (tdoa_process_locate_zoom)
        int zoom_cols = 1;                       // the fine grid's columns
        std::vector<tdoa_cell_track> ltracks;    // --locate-track: one record per block, a cell and its own score per stack
        std::vector<int32_t> lt_cells;           // (tdoa_process_locate_track)
        std::vector<int64_t> lt_own;
        std::vector<tdoa_cell_track> ztracks;    // --locate-track-zoom: one more record per block, a fine cell per stack
        std::vector<int32_t> zt_cells;           // (tdoa_process_locate_track_zoom)
        int tzoom_cols = 1;                      // its fine grid's columns
        std::vector<tdoa_location> mlocs;        // --emitters: one record per round and stack (tdoa_process_locate_multi)
        std::vector<tdoa_zoom> mzooms;           // --zoom-emitters: one more record and its counts per round and stack
        std::vector<int32_t> mzpairs;            // (tdoa_process_locate_multi_zoom)
        std::vector<tdoa_cell_track> mtracks;    // --track-emitters: one record per round and block, a cell, its own score and the
        std::vector<int32_t> mt_cells, mt_pairs; // pairs' counts per round and stack (tdoa_process_locate_track_multi)
        std::vector<int64_t> mt_own;
        std::vector<tdoa_map_stats> lstats, mstats, ltstats, mtstats;      // --map-stats: one record per record of the four above
        std::vector<tdoa_sync> syncs;            // --sync: one record and S clocks per block (tdoa_process_sync)
        std::vector<int32_t> clocks;
        std::vector<int32_t> ref16;              // --one-call: the reference emitter's delays, kept for the one call
        std::vector<tdoa_sync> sfines;           // --sync-fine: one more record and S clocks in 1/16 sample per block (tdoa_process_sync_fine)
        std::vector<int32_t> clocks16;
        std::vector<tdoa_sync_line> lines;       // --sync-drift: one record, S clocks and S rates per block (tdoa_process_sync_drift)
        std::vector<int32_t> rates;
        std::vector<tdoa_sync_line> flines;      // --sync-drift-fine: one more record, S clocks in 1/16 sample and S fine rates per block
        std::vector<int32_t> fclocks16, frates;
        double grid_lat0 = 0, grid_lon0 = 0, grid_dlat = 0, grid_dlon = 0;
        if (stack) {
            if ((rc = tdoa_num_stacks(ctx, stack_m, &spb, &n_stacks))) return die("tdoa_num_stacks", rc);
            stacks = Stacks(wpb, stack_m, spb, n_stacks);
            spk.resize((size_t)n_stacks * P * 2);
            scnt.resize((size_t)n_stacks * P);
            sfine.resize((size_t)n_stacks * P);
            if (drift) {
                sdrift.resize((size_t)n_stacks * P);
                if ((rc = tdoa_process_stacked_drift(ctx, stack_m, 2, 1, gate, drift_h, drift_d, spk.data(), scnt.data(), sfine.data(),
                                                     nullptr, nullptr, sdrift.data(), nullptr)))
                    return die("tdoa_process_stacked_drift", rc);
            } else if ((rc = tdoa_process_stacked(ctx, 0, 1, stack_m, 2, 1, gate, spk.data(), scnt.data(), sfine.data(), nullptr, nullptr)))
                return die("tdoa_process_stacked", rc);
            if (track) {
                tscore.resize((size_t)n_stacks * P);
                tlags.resize((size_t)n_stacks * P * stacks.m);
                if ((rc = tdoa_process_track(ctx, stack_m, track_j, tscore.data(), tlags.data(), nullptr, nullptr, nullptr)))
                    return die("tdoa_process_track", rc);
            }
            if (closure) {
                clos.resize((size_t)n_stacks * std::max(tdoa_num_triples(ctx), 1));
                if ((rc = tdoa_process_closure(ctx, stack_m, closure_g, closure_sep, nullptr, clos.data())))
                    return die("tdoa_process_closure", rc);
            }
            if (locate) {
                // the grid: SPAN_KM on a side around the stations' centroid, a degree of latitude taken as 111.32 km and a
                // degree of longitude as 111.32 km cos(latitude of the centroid)
                std::vector<double> lle(3 * (size_t)S);
                double lat_c = 0, lon_c = 0, h_c = 0;
                for (int s = 0; s < S; s++) {
                    lat_c += (lle[3 * s] = caps[s].st.lat) / S;
                    lon_c += (lle[3 * s + 1] = caps[s].st.lon) / S;
                    h_c += (lle[3 * s + 2] = caps[s].st.elev) / S;
                }
                const double pi = 3.14159265358979323846, span_lat = locate_km / 111.32, span_lon = locate_km / (111.32 * std::cos(lat_c * pi / 180));
                grid_dlat = locate_rows > 1 ? span_lat / (locate_rows - 1) : 0.0;
                grid_dlon = locate_cols > 1 ? span_lon / (locate_cols - 1) : 0.0;
                grid_lat0 = lat_c - grid_dlat * (locate_rows - 1) / 2;
                grid_lon0 = lon_c - grid_dlon * (locate_cols - 1) / 2;
                std::vector<int32_t> table((size_t)locate_rows * locate_cols * S);
                if ((rc = tdoa_locate_grid_table(lle.data(), S, grid_lat0, grid_lon0, grid_dlat, grid_dlon, locate_rows, locate_cols, h_c,
                                                 prm.sample_rate, table.data())))
                    return die("tdoa_locate_grid_table", rc);
                if ((rc = tdoa_locate_set_table(ctx, table.data(), locate_rows * locate_cols, locate_cols, S)))
                    return die("tdoa_locate_set_table", rc);
                if (sync) {
                    // the known emitter's delays: the table of its one cell; then the clocks of every block (the blocks are
                    // the stacks here), and the locate's clock table from those of the two reference blocks
                    std::vector<int32_t> ref((size_t)S), table16((size_t)n_stacks * S);
                    if ((rc = tdoa_locate_grid_table(lle.data(), S, sync_lat, sync_lon, 0.0, 0.0, 1, 1, sync_h, prm.sample_rate, ref.data())))
                        return die("tdoa_locate_grid_table", rc);
                    if (sync_drift) {
                        // the lines of the three blocks and their rows; the target block's rows are block 1's line continued
                        lines.resize(3);
                        clocks.resize(3 * (size_t)S);
                        rates.resize(3 * (size_t)S);
                        if (one_call) {
                            ref16 = ref;                     // the lines are searched with the zoomed tracks, below
                        } else if (sync_drift_fine) {               // the fine rows; the target block's are block 1's fine line continued
                            flines.resize(3);
                            fclocks16.resize(3 * (size_t)S);
                            frates.resize(3 * (size_t)S);
                            if ((rc = tdoa_process_sync_drift_fine(ctx, stack_m, sync_g, sdrift_h, sdrift_d, sync_r, sdfine_u, sdfine_r, ref.data(),
                                                                   nullptr, lines.data(), clocks.data(), rates.data(), nullptr, nullptr, nullptr,
                                                                   flines.data(), fclocks16.data(), frates.data(), table16.data(), nullptr, nullptr)))
                                return die("tdoa_process_sync_drift_fine", rc);
                            if ((rc = tdoa_sync_line_clock16(fclocks16.data(), frates.data(), S, sdfine_u, sdrift_d, spb, spb,
                                                             table16.data() + (size_t)spb * S)))
                                return die("tdoa_sync_line_clock16", rc);
                        } else {
                            if ((rc = tdoa_process_sync_drift(ctx, stack_m, sync_g, sdrift_h, sdrift_d, sync_r, ref.data(), nullptr, lines.data(),
                                                              clocks.data(), rates.data(), table16.data(), nullptr, nullptr)))
                                return die("tdoa_process_sync_drift", rc);
                            if ((rc = tdoa_sync_line_clock(clocks.data(), rates.data(), S, sdrift_d, spb, spb, table16.data() + (size_t)spb * S)))
                                return die("tdoa_sync_line_clock", rc);
                        }
                    } else if (one_call) {
                        ref16 = ref;                         // the clocks are searched with the zoom locate, below
                    } else if (sync_fine) {
                        syncs.resize((size_t)n_stacks);
                        clocks.resize((size_t)n_stacks * S);
                        sfines.resize((size_t)n_stacks);
                        clocks16.resize((size_t)n_stacks * S);
                        if ((rc = tdoa_process_sync_fine(ctx, stack_m, sync_g, sync_r, sfine_u, sfine_r, ref.data(), nullptr, syncs.data(), clocks.data(),
                                                         nullptr, nullptr, sfines.data(), clocks16.data(), nullptr, nullptr)))
                            return die("tdoa_process_sync_fine", rc);
                        for (int s = 0; s < S; s++) {            // the midpoint: the nearest integer to (a + b) / 2, halves away from zero
                            const long long before = clocks16[s], after = clocks16[2 * (size_t)S + s], t = before + after;
                            table16[s] = (int32_t)before;
                            table16[(size_t)S + s] = (int32_t)(t < 0 ? -((-t + 1) / 2) : (t + 1) / 2);
                            table16[2 * (size_t)S + s] = (int32_t)after;
                        }
                    } else {
                        syncs.resize((size_t)n_stacks);
                        clocks.resize((size_t)n_stacks * S);
                        if ((rc = tdoa_process_sync(ctx, stack_m, sync_g, sync_r, ref.data(), nullptr, syncs.data(), clocks.data(), nullptr, nullptr)))
                            return die("tdoa_process_sync", rc);
                        for (int s = 0; s < S; s++) {
                            const int32_t before = clocks[s], after = clocks[2 * (size_t)S + s];
                            table16[s] = TDOA_DELAY_UNIT * before;
                            table16[(size_t)S + s] = TDOA_DELAY_UNIT / 2 * (before + after);
                            table16[2 * (size_t)S + s] = TDOA_DELAY_UNIT * after;
                        }
                    }
                    if (!one_call && (rc = tdoa_locate_set_clock(ctx, table16.data(), n_stacks, S))) return die("tdoa_locate_set_clock", rc);
                }
                if ((rc = tdoa_locate_set_upsample(ctx, locate_up))) return die("tdoa_locate_set_upsample", rc);
                if (map_stats && (rc = tdoa_locate_set_stats(ctx, stats_ranks.data(), (int)stats_ranks.size(), stats_foot)))
                    return die("tdoa_locate_set_stats", rc);
                const auto last_stats = [&](std::vector<tdoa_map_stats> *out, size_t n) {
                    out->resize(map_stats ? n : 0);
                    return map_stats ? tdoa_locate_last_stats(ctx, out->data(), (int)n, nullptr) : TDOA_OK;
                };
                if (one_call && sync_drift_fine) {
                    // The fine lines, the rows and the zoomed tracks in one call, on the fine grid --locate-track-zoom builds below:
                    // blocks 1 and 3 their own lines at their own positions, stack j of block 2 block 1's fine line continued to
                    // spb + j.  The rows then go to the clock table for the searches further down, which this call itself never reads
                    const int rows_f = (locate_rows - 1) * tzoom_z + 1;
                    tzoom_cols = (locate_cols - 1) * tzoom_z + 1;
                    std::vector<int32_t> fine((size_t)rows_f * tzoom_cols * S);
                    if ((rc = tdoa_locate_grid_table(lle.data(), S, grid_lat0, grid_lon0, grid_dlat / tzoom_z, grid_dlon / tzoom_z, rows_f, tzoom_cols,
                                                     h_c, prm.sample_rate, fine.data())))
                        return die("tdoa_locate_grid_table", rc);
                    if ((rc = tdoa_locate_set_fine_table(ctx, fine.data(), rows_f * tzoom_cols, tzoom_cols, S))) return die("tdoa_locate_set_fine_table", rc);
                    std::vector<tdoa_line_mix> mix((size_t)n_stacks);
                    for (int t = 0; t < n_stacks; t++)
                        mix[t] = t / spb == 1 ? tdoa_line_mix{0, t, 0, t, 1, 0} : tdoa_line_mix{t / spb, t % spb, t / spb, t % spb, 1, 0};
                    std::vector<int32_t> rows16((size_t)n_stacks * S);
                    flines.resize(3);
                    fclocks16.resize(3 * (size_t)S);
                    frates.resize(3 * (size_t)S);
                    ltracks.resize((size_t)(n_stacks / spb));
                    lt_cells.resize((size_t)n_stacks);
                    lt_own.resize((size_t)n_stacks);
                    ztracks.resize(ltracks.size());
                    zt_cells.resize((size_t)n_stacks);
                    if ((rc = tdoa_process_sync_drift_locate(ctx, stack_m, sync_g, sdrift_h, sdrift_d, sync_r, sdfine_u, sdfine_r, ref16.data(), nullptr,
                                                             mix.data(), ltrack_j, ltrack_sep, tzoom_z, tzoom_h, tzoom_jf, tzoom_sep, lines.data(),
                                                             clocks.data(), rates.data(), nullptr, nullptr, nullptr, flines.data(), fclocks16.data(),
                                                             frates.data(), nullptr, nullptr, nullptr, rows16.data(), ltracks.data(), lt_cells.data(),
                                                             lt_own.data(), nullptr, nullptr, nullptr, ztracks.data(), zt_cells.data(), nullptr, nullptr,
                                                             nullptr, nullptr, nullptr)))
                        return die("tdoa_process_sync_drift_locate", rc);
                    if ((rc = last_stats(&ltstats, ltracks.size()))) return die("tdoa_locate_last_stats", rc);
                    if ((rc = tdoa_locate_set_clock(ctx, rows16.data(), n_stacks, S))) return die("tdoa_locate_set_clock", rc);
                }
                locs.resize((size_t)n_stacks);
                if (locate_zoom) {
                    // the same grid at Z cells per cell: fine cell (Z r, Z c) lies where cell (r, c) does
                    const int rows_f = (locate_rows - 1) * zoom_z + 1;
                    zoom_cols = (locate_cols - 1) * zoom_z + 1;
                    std::vector<int32_t> fine((size_t)rows_f * zoom_cols * S);
                    if ((rc = tdoa_locate_grid_table(lle.data(), S, grid_lat0, grid_lon0, grid_dlat / zoom_z, grid_dlon / zoom_z, rows_f, zoom_cols, h_c,
                                                     prm.sample_rate, fine.data())))
                        return die("tdoa_locate_grid_table", rc);
                    if ((rc = tdoa_locate_set_fine_table(ctx, fine.data(), rows_f * zoom_cols, zoom_cols, S))) return die("tdoa_locate_set_fine_table", rc);
                    zooms.resize((size_t)n_stacks);
                    if (one_call && sync_fine) {
                        // blocks 1 and 3 their own refined clocks, stack j of block 2 the midpoint of stack j of blocks 1 and 3; the
                        // rows then go to the clock table for the searches further down, which this call itself never reads
                        std::vector<tdoa_clock_mix> mix((size_t)n_stacks);
                        for (int t = 0; t < n_stacks; t++)
                            mix[t] = t / spb == 1 ? tdoa_clock_mix{t - spb, t + spb, 1, 1} : tdoa_clock_mix{t, t, 1, 0};
                        std::vector<int32_t> rows16((size_t)n_stacks * S);
                        syncs.resize((size_t)n_stacks);
                        clocks.resize((size_t)n_stacks * S);
                        sfines.resize((size_t)n_stacks);
                        clocks16.resize((size_t)n_stacks * S);
                        if ((rc = tdoa_process_sync_locate(ctx, stack_m, sync_g, sync_r, sfine_u, sfine_r, ref16.data(), nullptr, mix.data(), 1, zoom_z,
                                                           zoom_h, zoom_sep, syncs.data(), clocks.data(), nullptr, nullptr, sfines.data(), clocks16.data(),
                                                           nullptr, nullptr, rows16.data(), locs.data(), nullptr, nullptr, nullptr, zooms.data(), nullptr,
                                                           nullptr, nullptr)))
                            return die("tdoa_process_sync_locate", rc);
                        if ((rc = last_stats(&lstats, locs.size()))) return die("tdoa_locate_last_stats", rc);
                        if ((rc = tdoa_locate_set_clock(ctx, rows16.data(), n_stacks, S))) return die("tdoa_locate_set_clock", rc);
                    } else if ((rc = tdoa_process_locate_zoom(ctx, stack_m, 1, zoom_z, zoom_h, zoom_sep, locs.data(), nullptr, nullptr, nullptr,
                                                              zooms.data(), nullptr, nullptr, nullptr)))
                        return die("tdoa_process_locate_zoom", rc);
                } else if ((rc = tdoa_process_locate(ctx, stack_m, 1, locs.data(), nullptr, nullptr, nullptr)))
                    return die("tdoa_process_locate", rc);
                if (!(one_call && sync_fine) && (rc = last_stats(&lstats, locs.size()))) return die("tdoa_locate_last_stats", rc);
                if (emitters) {
                    mlocs.resize((size_t)emitters_k * n_stacks);
                    if (zoom_emitters) {         // the rounds' records are tdoa_process_locate_multi's bytes
                        mzooms.resize(mlocs.size());
                        mzpairs.resize(2 * mlocs.size());
                        if ((rc = tdoa_process_locate_multi_zoom(ctx, stack_m, emitters_k, emitters_guard, 1, zoom_z, zoom_h, zoom_sep, mlocs.data(),
                                                                 nullptr, nullptr, nullptr, mzooms.data(), mzpairs.data(), nullptr, nullptr, nullptr)))
                            return die("tdoa_process_locate_multi_zoom", rc);
                    } else if ((rc = tdoa_process_locate_multi(ctx, stack_m, emitters_k, emitters_guard, 1, mlocs.data(), nullptr, nullptr, nullptr)))
                        return die("tdoa_process_locate_multi", rc);
                    if ((rc = last_stats(&mstats, mlocs.size()))) return die("tdoa_locate_last_stats", rc);
                }
                if (locate_track && !(one_call && sync_drift_fine)) {       // (the one call above has tracked already)
                    ltracks.resize((size_t)(n_stacks / spb));
                    lt_cells.resize((size_t)n_stacks);
                    lt_own.resize((size_t)n_stacks);
                    if (track_zoom) {
                        // the same grid at Z cells per cell, as --locate-zoom builds it (this call's Z: the fine table is set anew)
                        const int rows_f = (locate_rows - 1) * tzoom_z + 1;
                        tzoom_cols = (locate_cols - 1) * tzoom_z + 1;
                        std::vector<int32_t> fine((size_t)rows_f * tzoom_cols * S);
                        if ((rc = tdoa_locate_grid_table(lle.data(), S, grid_lat0, grid_lon0, grid_dlat / tzoom_z, grid_dlon / tzoom_z, rows_f,
                                                         tzoom_cols, h_c, prm.sample_rate, fine.data())))
                            return die("tdoa_locate_grid_table", rc);
                        if ((rc = tdoa_locate_set_fine_table(ctx, fine.data(), rows_f * tzoom_cols, tzoom_cols, S)))
                            return die("tdoa_locate_set_fine_table", rc);
                        ztracks.resize(ltracks.size());
                        zt_cells.resize((size_t)n_stacks);
                        if ((rc = tdoa_process_locate_track_zoom(ctx, stack_m, ltrack_j, ltrack_sep, tzoom_z, tzoom_h, tzoom_jf, tzoom_sep, ltracks.data(),
                                                                 lt_cells.data(), lt_own.data(), nullptr, nullptr, nullptr, ztracks.data(),
                                                                 zt_cells.data(), nullptr, nullptr, nullptr, nullptr, nullptr)))
                            return die("tdoa_process_locate_track_zoom", rc);
                    } else if ((rc = tdoa_process_locate_track(ctx, stack_m, ltrack_j, ltrack_sep, ltracks.data(), lt_cells.data(), lt_own.data(),
                                                               nullptr, nullptr, nullptr)))
                        return die("tdoa_process_locate_track", rc);
                    if ((rc = last_stats(&ltstats, ltracks.size()))) return die("tdoa_locate_last_stats", rc);
                }
                if (track_emitters) {
                    mtracks.resize((size_t)temitters_k * (n_stacks / spb));
                    mt_cells.resize((size_t)temitters_k * n_stacks);
                    mt_own.resize((size_t)temitters_k * n_stacks);
                    mt_pairs.resize((size_t)temitters_k * n_stacks * 2);
                    if ((rc = tdoa_process_locate_track_multi(ctx, stack_m, ltrack_j, temitters_k, temitters_guard, ltrack_sep, mtracks.data(),
                                                              mt_cells.data(), mt_own.data(), mt_pairs.data(), nullptr, nullptr, nullptr)))
                        return die("tdoa_process_locate_track_multi", rc);
                    if ((rc = last_stats(&mtstats, mtracks.size()))) return die("tdoa_locate_last_stats", rc);
                }
            }
        }
        std::printf("\n=== FM-DISCRIMINATOR CROSS-CORRELATION: %d windows x %d pairs ===\n", W, P);
        int p = 0;
        for (int i = 0; i < S; i++)
            for (int j = i + 1; j < S; j++, p++) {
                std::vector<double> lr, lt, cr, ct;
                for (int w = 0; w < W; w++) {
                    const tdoa_peak &pk = peaks[(size_t)w * P + p];
                    const bool target = (w / wpb) == 1;        // block 1 is the target frequency
                    (target ? lt : lr).push_back(pk.lag);
                    (target ? ct : cr).push_back(std::fabs(pk.corr));
                }
                std::printf("REF %s - %s: median lag=%.0f samples over %zu windows, median |corr|=%.6f\n", caps[i].st.name.c_str(),
                            caps[j].st.name.c_str(), median(lr), lr.size(), median(cr));
                std::printf("TGT %s - %s: median lag=%.0f samples over %zu windows, median |corr|=%.6f\n", caps[i].st.name.c_str(),
                            caps[j].st.name.c_str(), median(lt), lt.size(), median(ct));
                double lag_used = median(lt);
                if (fine) {
                    // refined delays of the target windows that pass the gate (all of them if none does)
                    std::vector<double> ok, all;
                    for (int w = 0; w < W; w++) {
                        if ((w / wpb) != 1) continue;
                        const tdoa_fine_peak &fk = fines[(size_t)w * P + p];
                        all.push_back(fk.delay);
                        if (fk.plausible) ok.push_back(fk.delay);
                    }
                    lag_used = median(ok.empty() ? all : ok);
                    if (ok.empty()) ct.clear();                    // no plausible window: the pair gets weight 0 in the N-station solve
                    std::printf("TGT %s - %s: refined delay=%.3f samples, %zu of %zu windows within +-%.1f samples\n",
                                caps[i].st.name.c_str(), caps[j].st.name.c_str(), lag_used, ok.size(), all.size(), gate);
                }
                if (stack) {
                    // one line per stack; the target block's refined stacked delays replace the per-window choice
                    std::vector<double> sd, sc;
                    for (int sid = 0; sid < n_stacks; sid++) {
                        const size_t u = (size_t)sid * P + p;
                        const tdoa_peak &p1 = spk[2 * u], &p2 = spk[2 * u + 1];
                        const int sj = sid % spb, n_w = stacks.n_w(sid);
                        std::printf("STACK block %d stack %d %s - %s: windows=%d delay=%d samples refined=%.3f |C|=%.6f ratio=%.3f",
                                    sid / spb + 1, sj, caps[i].st.name.c_str(), caps[j].st.name.c_str(), n_w, p1.lag,
                                    sfine[u].delay, (double)p1.abs_corr,
                                    scnt[u] > 1 ? (double)p1.abs_corr / (double)p2.abs_corr : INFINITY);
                        if (drift)               // the slope h* / D and the relative clock rate it stands for
                            std::printf(" drift=%+d/%d lags/window (%+.3f ppm)", (int)sdrift[u], drift_d,
                                        1e6 * (double)sdrift[u] / ((double)drift_d * (double)wlen));
                        std::printf("\n");
                        if (sid / spb == 1) { sd.push_back(sfine[u].delay); sc.push_back(p1.abs_corr); }
                    }
                    for (int sid = 0; track && sid < n_stacks; sid++) {   // the track of every stack: a line of its own
                        const size_t u = (size_t)sid * P + p;
                        const int sj = sid % spb, n_w = stacks.n_w(sid);
                        const int32_t *lg = tlags.data() + u * stacks.m;
                        std::printf("TRACK block %d stack %d %s - %s: windows=%d step=%d first=%d last=%d score=%.6f lags=",
                                    sid / spb + 1, sj, caps[i].st.name.c_str(), caps[j].st.name.c_str(), n_w, track_j, (int)lg[0],
                                    (int)lg[n_w - 1], tscore[u].corr);
                        for (int w = 0; w < n_w; w++) std::printf(w ? ",%d" : "%d", (int)lg[w]);
                        std::printf("\n");
                    }
                    lag_used = median(sd);
                    ct = sc;
                }
                tgt_dt.push_back(lag_used / prm.sample_rate);
                tgt_w.push_back(median(ct));
            }
        // --closure: the three lags of every station triple that close, a line per stack and triple
        const int T = closure ? tdoa_num_triples(ctx) : 0;
        for (int sid = 0; sid < (T ? n_stacks : 0); sid++) {
            const double root = std::sqrt((double)stacks.n_w(sid));
            int t = 0;
            for (int i = 0; i < S; i++)
                for (int j = i + 1; j < S; j++)
                    for (int k = j + 1; k < S; k++, t++) {
                        const tdoa_closure &c = clos[(size_t)sid * T + t];
                        std::printf("CLOSURE block %d stack %d %s - %s - %s: lags=%d,%d,%d residual=%d score=%.6f own=%.6f runner=%.6f\n",
                                    sid / spb + 1, sid % spb, caps[i].st.name.c_str(), caps[j].st.name.c_str(), caps[k].st.name.c_str(),
                                    (int)c.lag_ij, (int)c.lag_ik, (int)c.lag_jk, (int)c.residual, c.score,
                                    (double)c.own_q / 4294967296.0 / root, c.runner_up);
                    }
        }
        // --sync: the clocks of the two reference blocks, a line each
        for (size_t sid = 0; sid < syncs.size(); sid += 2) {
            std::printf("SYNC block %d: clock=", (int)sid + 1);
            for (int s = 0; s < S; s++) std::printf("%s%d", s ? "," : "", (int)clocks[sid * S + s]);
            std::printf(" moved=%d score=%.6f\n", (int)syncs[sid].moved, syncs[sid].score);
        }
        // --sync-fine: the refined clocks of the two reference blocks in 1/16 sample, a line each
        for (size_t sid = 0; sid < sfines.size(); sid += 2) {
            std::printf("SYNCFINE block %d: clock16=", (int)sid + 1);
            for (int s = 0; s < S; s++) std::printf("%s%d", s ? "," : "", (int)clocks16[sid * S + s]);
            std::printf(" moved=%d score=%.6f\n", (int)sfines[sid].moved, sfines[sid].score);
        }
        // --sync-drift: the lines of the two reference blocks, a line each
        for (size_t b = 0; b < lines.size(); b += 2) {
            std::printf("SYNCLINE block %d: clock=", (int)b + 1);
            for (int s = 0; s < S; s++) std::printf("%s%d", s ? "," : "", (int)clocks[b * S + s]);
            std::printf(" rate=");
            for (int s = 0; s < S; s++) std::printf("%s%d", s ? "," : "", (int)rates[b * S + s]);
            std::printf("/%d moved=%d score=%.6f\n", sdrift_d, (int)lines[b].moved, lines[b].score);
        }
        // --sync-drift-fine: the fine lines of the two reference blocks, a line each
        for (size_t b = 0; b < flines.size(); b += 2) {
            std::printf("SYNCLINEFINE block %d: clock16=", (int)b + 1);
            for (int s = 0; s < S; s++) std::printf("%s%d", s ? "," : "", (int)fclocks16[b * S + s]);
            std::printf(" fine_rate=");
            for (int s = 0; s < S; s++) std::printf("%s%d", s ? "," : "", (int)frates[b * S + s]);
            std::printf("/%d moved=%d score=%.6f\n", sdfine_u * sdrift_d, (int)flines[b].moved, flines[b].score);
        }
        // --map-stats: the statistics of the plane the line before it judged, the words on the line's own scale
        const auto print_stats = [&](const std::vector<tdoa_map_stats> &all, size_t at) {
            if (at >= all.size()) return;
            const tdoa_map_stats &m = all[at];
            const double scale = m.quantile_q[0] ? m.quantile[0] / (double)m.quantile_q[0] : 0.0;
            std::printf("STATS live=%d q=", (int)m.n_live);
            for (size_t r = 0; r < stats_ranks.size(); r++) std::printf("%s%.6f", r ? "," : "", m.quantile[r]);
            std::printf(" level=%.6f foot=%d near=%d rows=%d..%d cols=%d..%d\n", (double)m.level_q * scale, (int)m.foot_cells, (int)m.foot_near,
                        (int)m.row_lo, (int)m.row_hi, (int)m.col_lo, (int)m.col_hi);
        };
        // --locate: the best cell of the grid, a line per stack
        for (size_t sid = 0; sid < locs.size(); sid++) {
            const tdoa_location &l = locs[sid];
            std::printf("LOCATE block %d stack %d: cell=%d lat=%.6f lon=%.6f pairs=%d score=%.6f runner=%.6f\n", (int)sid / spb + 1,
                        (int)sid % spb, (int)l.cell, grid_lat0 + (l.cell / locate_cols) * grid_dlat, grid_lon0 + (l.cell % locate_cols) * grid_dlon,
                        (int)l.pairs_in, l.score, l.runner_up);
            print_stats(lstats, sid);
            if (locate_zoom) {               // the fine cell, its plateau's box in fine rows and columns, the runner-up; cell=-1: none
                const tdoa_zoom &z = zooms[sid];
                const int cell = z.score_q > 0 ? (int)z.cell : -1;
                std::printf("ZOOM block %d stack %d: cell=%d lat=%.6f lon=%.6f pairs=%d score=%.6f best=%d rows=%d..%d cols=%d..%d runner=%.6f runner_cell=%d\n",
                            (int)sid / spb + 1, (int)sid % spb, cell, grid_lat0 + (z.cell / zoom_cols) * grid_dlat / zoom_z,
                            grid_lon0 + (z.cell % zoom_cols) * grid_dlon / zoom_z, (int)z.pairs_in, z.score, (int)z.n_best, (int)z.row_lo, (int)z.row_hi,
                            (int)z.col_lo, (int)z.col_hi, z.runner_up, (int)z.runner_cell);
            }
        }
        // --emitters: a fix per round, the stack's rounds together; a round that found nothing prints cell=-1
        for (size_t sid = 0; sid < mlocs.size() / (size_t)emitters_k; sid++)
            for (int r = 0; r < emitters_k; r++) {
                const tdoa_location &l = mlocs[(size_t)r * n_stacks + sid];
                const int cell = l.score_q > 0 ? (int)l.cell : -1;
                std::printf("LOCATE-MULTI block %d stack %d round %d: cell=%d lat=%.6f lon=%.6f pairs=%d excluded=%d score=%.6f runner=%.6f\n",
                            (int)sid / spb + 1, (int)sid % spb, r, cell, grid_lat0 + (l.cell / locate_cols) * grid_dlat,
                            grid_lon0 + (l.cell % locate_cols) * grid_dlon, (int)l.pairs_in, (int)l.reserved, l.score, l.runner_up);
                print_stats(mstats, (size_t)r * n_stacks + sid);
            }
        // --zoom-emitters: every round's fine cell, the ZOOM line's fields and the pairs excluded there; cell=-1: none
        for (size_t sid = 0; sid < mzooms.size() / (size_t)emitters_k; sid++)
            for (int r = 0; r < emitters_k; r++) {
                const size_t at = (size_t)r * n_stacks + sid;
                const tdoa_zoom &z = mzooms[at];
                const int cell = z.score_q > 0 ? (int)z.cell : -1;
                std::printf("EMITTER-ZOOM block %d stack %d round %d: cell=%d lat=%.6f lon=%.6f pairs=%d score=%.6f best=%d rows=%d..%d cols=%d..%d "
                            "runner=%.6f runner_cell=%d reserved=%d\n",
                            (int)sid / spb + 1, (int)sid % spb, r, cell, grid_lat0 + (z.cell / zoom_cols) * grid_dlat / zoom_z,
                            grid_lon0 + (z.cell % zoom_cols) * grid_dlon / zoom_z, (int)z.pairs_in, z.score, (int)z.n_best, (int)z.row_lo, (int)z.row_hi,
                            (int)z.col_lo, (int)z.col_hi, z.runner_up, (int)z.runner_cell, (int)mzpairs[2 * at + 1]);
            }
        // --locate-track: the block's track, then its cell in every stack with the stack's own score there (on the stack's scale)
        for (size_t b = 0; b < ltracks.size(); b++) {
            const tdoa_cell_track &t = ltracks[b];
            std::printf("LOCATE-TRACK block %d: cell=%d positions=%d steps=%d score=%.6f runner=%.6f runner_cell=%d\n", (int)b + 1, (int)t.cell,
                        (int)t.positions, (int)t.steps, t.score, t.runner_up, (int)t.runner_cell);
            print_stats(ltstats, b);
            for (int j = 0; j < spb; j++) {
                const size_t sid = b * spb + j;
                const int cell = lt_cells[sid];
                std::printf("LOCATE-TRACK block %d stack %d: cell=%d lat=%.6f lon=%.6f own=%.6f\n", (int)b + 1, j, cell,
                            grid_lat0 + (cell / locate_cols) * grid_dlat, grid_lon0 + (cell % locate_cols) * grid_dlon,
                            (double)lt_own[sid] / 4294967296.0 / std::sqrt((double)stacks.n_w((int)sid)));
            }
            if (track_zoom) {                // the fine track: its first fine cell and where that lies, then every stack's; cell=-1: none
                const tdoa_cell_track &z = ztracks[b];
                std::printf("TRACKZOOM block %d: cell=%d lat=%.6f lon=%.6f positions=%d steps=%d score=%.6f runner=%.6f runner_cell=%d cells=",
                            (int)b + 1, z.score_q > 0 ? (int)z.cell : -1, grid_lat0 + (z.cell / tzoom_cols) * grid_dlat / tzoom_z,
                            grid_lon0 + (z.cell % tzoom_cols) * grid_dlon / tzoom_z, (int)z.positions, (int)z.steps, z.score, z.runner_up,
                            (int)z.runner_cell);
                for (int j = 0; j < spb; j++) std::printf("%s%d", j ? "," : "", (int)zt_cells[b * spb + j]);
                std::printf("\n");
            }
        }
        // --track-emitters: a track per block and round, the block's rounds together, each followed by its positions; a round
        // that found nothing prints cell=-1
        const size_t n_blocks = mtracks.empty() ? 0 : (size_t)(n_stacks / spb);
        for (size_t b = 0; b < n_blocks; b++)
            for (int r = 0; r < temitters_k; r++) {
                const tdoa_cell_track &t = mtracks[(size_t)r * n_blocks + b];
                const bool found = t.score_q > 0;
                std::printf("LOCATE-TRACK-MULTI block %d round %d: cell=%d positions=%d steps=%d score=%.6f runner=%.6f runner_cell=%d\n",
                            (int)b + 1, r, found ? (int)t.cell : -1, (int)t.positions, (int)t.steps, t.score, t.runner_up, (int)t.runner_cell);
                print_stats(mtstats, (size_t)r * n_blocks + b);
                for (int j = 0; j < spb; j++) {
                    const size_t sid = b * spb + j, at = (size_t)r * n_stacks + sid;
                    const int cell = mt_cells[at];
                    std::printf("LOCATE-TRACK-MULTI block %d round %d stack %d: cell=%d lat=%.6f lon=%.6f own=%.6f pairs=%d excluded=%d\n",
                                (int)b + 1, r, j, found ? cell : -1, grid_lat0 + (cell / locate_cols) * grid_dlat,
                                grid_lon0 + (cell % locate_cols) * grid_dlon,
                                (double)mt_own[at] / 4294967296.0 / std::sqrt((double)stacks.n_w((int)sid)), (int)mt_pairs[2 * at],
                                (int)mt_pairs[2 * at + 1]);
                }
            }
    }

    // ---- downstream: range differences and the position solve (processor.go:892-926)
    std::vector<double> rd(tgt_dt.size());
    std::printf("\n=== TDOA GEOLOCATION ===\nTime differences (μs): ");
    for (size_t i = 0; i < tgt_dt.size(); i++) { rd[i] = tgt_dt[i] * kC; std::printf("%.3f ", tgt_dt[i] * 1e6); }
    std::printf("\nRange differences (m): ");
    for (double v : rd) std::printf("%.1f ", v);
    std::printf("\n");
    std::vector<double> lle(3 * S);
    for (int s = 0; s < S; s++) { lle[3 * s] = caps[s].st.lat; lle[3 * s + 1] = caps[s].st.lon; lle[3 * s + 2] = caps[s].st.elev; }
    double out[3];
    int iters = 0;
    if (S == 3) rc = tdoa_solve_3station(lle.data(), rd.data(), out, &iters);
    else rc = tdoa_solve_nstation(lle.data(), S, rd.data(), tgt_w.data(), 0, out, &iters);   // weights: median |corr| per pair
    if (rc != TDOA_OK) {                                       // processor.go:919-921
        if (rc == TDOA_ERR_INVALID)
            std::fprintf(stderr, "TDOA solution failed: fewer usable station pairs than unknowns (no target window of the "
                                 "other pairs passed the +-%.1f-sample plausibility gate, or a weight is not finite)\n", gate);
        else
            std::fprintf(stderr, "TDOA solution failed: %s at iteration %d\n", tdoa_strerror(rc), iters);
        tdoa_destroy(ctx);
        return 3;
    }
    std::printf("\n*** CALCULATED TRANSMITTER LOCATION ***\nLatitude:  %.6f°\nLongitude: %.6f°\nElevation: %.1f m\n", out[0], out[1], out[2]);
    tdoa_destroy(ctx);
    return 0;
}
