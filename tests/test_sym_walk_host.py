"""Host-side check of the walk of the symmetric sweeps (csrc/sym_walk.h: sym_walk).  The walk is plain integer arithmetic
above the header's __HIPCC__ block, so it is included in a host program (g++, `__device__` defined away) and run with a
body that records every hook call, for every wave of a launch.  The record of a wave is then replayed against the chunk
arithmetic restated here and unit_seek alone (no unit_next, no walk code):

  * every step of [step_begin, step_end) is consumed exactly once over all waves;
  * every unit(I, J, k0, k1, u) has (I, J) = unit_seek(order, u) and covers the steps [64 u + k0, 64 u + k1) the chunk
    has at that place;
  * load_row(I) comes before the first unit of every run of equal I and again after every begin(), never otherwise;
  * every load_row is matched by exactly one flush_row, whose argument is the unit before the row change, or the last
    unit of the chunk -- without a cull mask the last unit handed to unit();
  * a culled unit consumes its steps and gets neither load_row nor unit."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "rigidmultiblobswall_amd", "csrc")
PRELUDE = ("#include <cmath>\n#include <cstdio>\n#include <vector>\n"
           "#define __device__\n#define __host__\n#define __forceinline__ inline\n#include \"sym_walk.h\"\nusing namespace rmb;\n")

HARNESS = r'''
enum { BEGIN, VISIT, LOAD, FLUSH, UNIT };
struct Event { int kind, I, J, k0, k1; long u; };

static bool masked(int I, int J) {     // a fixed pseudo-random third of the off-diagonal units
  return I != J && (((unsigned)I * 2654435761u ^ (unsigned)J * 40503u) >> 7) % 3u == 0u;
}

struct Recorder {
  bool cull;
  std::vector<Event> ev;
  void begin() { ev.push_back({BEGIN, 0, 0, 0, 0, 0}); }
  bool culled(int I, int J) { const bool c = cull && masked(I, J); ev.push_back({VISIT, I, J, c, 0, 0}); return c; }
  void load_row(int I) { ev.push_back({LOAD, I, 0, 0, 0, 0}); }
  void flush_row(long u) { ev.push_back({FLUSH, 0, 0, 0, 0, u}); }
  void unit(int I, int J, int k0, int k1, long u) { ev.push_back({UNIT, I, J, k0, k1, u}); }
};

static long bad = 0;
#define CHECK(c) do { if (!(c)) { if (++bad < 20) printf("line %d: T %d order %d waves %ld spw %ld [%ld, %ld) cull %d wave %ld\n", __LINE__, T, order, n_waves, spw, b, e, (int)cull, w); } } while (0)

static void run(int T, int order, long n_waves, long spw, long b, long e, bool cull) {
  std::vector<int> seen(e - b, 0);
  long chunks = 0;
  Recorder rec;
  rec.cull = cull;
  for (long w = 0; w < n_waves; ++w) {
    rec.ev.clear();
    sym_walk(SymWalk{order, T, b, e, spw, n_waves, w}, rec);
    long chunk = w - n_waves, p = 0, p_end = 0, last_unit = -1;
    bool loaded = false;
    int cur_I = -1;
    const size_t n = rec.ev.size();
    for (size_t x = 0; x < n; ++x) {
      const Event& v = rec.ev[x];
      if (v.kind == BEGIN) {
        CHECK(p == p_end && !loaded);          // the chunk before was walked to its end and flushed
        chunk += n_waves; ++chunks;
        p = b + chunk * spw; p_end = p + spw < e ? p + spw : e;
        CHECK(p < e);
        cur_I = -1; last_unit = -1;
      } else if (v.kind == VISIT) {
        CHECK(p < p_end);
        const long u = p >> 6;
        int I, J; unit_seek(order, u, T, I, J);
        CHECK(v.I == I && v.J == J);
        const int k0 = (int)(p & 63);
        const int k1 = p_end - p < 64 - k0 ? (int)(k0 + (p_end - p)) : 64;
        for (long s = p; s < p + (k1 - k0); ++s) ++seen[s - b];
        p += k1 - k0;
        const bool is_culled = v.k0 != 0;
        CHECK(is_culled == (cull && masked(I, J)));
        size_t y = x + 1;
        if (is_culled) {                        // neither call; a flush may follow only as the chunk's last
          CHECK(y == n || rec.ev[y].kind == VISIT || rec.ev[y].kind == BEGIN || (rec.ev[y].kind == FLUSH && p == p_end));
          continue;
        }
        if (I != cur_I) {                       // row change, or the first unit after begin()
          if (loaded) {
            CHECK(y < n && rec.ev[y].kind == FLUSH && rec.ev[y].u == u - 1);
            if (!cull) CHECK(y < n && rec.ev[y].u == last_unit);
            loaded = false; ++y;
          }
          CHECK(y < n && rec.ev[y].kind == LOAD && rec.ev[y].I == I);
          loaded = true; cur_I = I; ++y;
        }
        CHECK(loaded);
        CHECK(y < n && rec.ev[y].kind == UNIT && rec.ev[y].I == I && rec.ev[y].J == J && rec.ev[y].k0 == k0 && rec.ev[y].k1 == k1 &&
              rec.ev[y].u == u);
        last_unit = u;
        x = y;
      } else if (v.kind == FLUSH) {             // the closing flush of a chunk (row changes are consumed above)
        CHECK(loaded && p == p_end && v.u == ((p_end - 1) >> 6));
        if (!cull) CHECK(v.u == last_unit);
        loaded = false;
      } else {
        CHECK(false);                           // a load or a unit that no visit accounts for
      }
    }
    CHECK(p == p_end && !loaded);
  }
  long w = -1;
  CHECK(chunks == (e - b + spw - 1) / spw);
  for (long s = 0; s < e - b; ++s) if (seen[s] != 1) { CHECK(false); break; }
}

int main() {
  std::vector<int> Ts;
  for (int T = 1; T <= 12; ++T) Ts.push_back(T);
  Ts.push_back(33); Ts.push_back(65);           // the first sizes with more than one super-block of the blocked order
  long runs = 0;
  for (int T : Ts) {
    const long S = 64L * T * (T + 1) / 2;
    const long c1 = (S / 3) | 1, c2 = (2 * S / 3) | 1;      // odd: no cut at a unit boundary
    const long ranges[4][2] = {{0, S}, {0, c1}, {c1, c2}, {c2, S}};
    for (int order = 0; order <= 1; ++order)
      for (long n_waves : {1L, 3L, 4L, 8L, 1000L})
        for (const auto& r : ranges) {
          const long steps = r[1] - r[0];
          for (long spw : {1L, 7L, 16L, 64L, 65L, 200L, (steps + n_waves - 1) / n_waves})
            for (int cull = 0; cull <= 1; ++cull) { run(T, order, n_waves, spw, r[0], r[1], cull != 0); ++runs; }
        }
  }
  printf("runs %ld problems %ld\n", runs, bad);
  return bad != 0;
}
'''


def test_sym_walk_hooks_and_step_coverage(tmp_path):
  cpp, exe = str(tmp_path / "sym_walk.cpp"), str(tmp_path / "sym_walk")
  with open(cpp, "w") as fh:
    fh.write(PRELUDE + HARNESS)
  subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", exe, cpp])
  res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
  assert res.returncode == 0 and "problems 0" in res.stdout, res.stdout + res.stderr
