// On-device game logic for the synthetic Atari-style suite (envs/atari_games.py):
// Breakout, SpaceInvaders, Alien / MsPacman, Centipede, and for the synthetic Doom scenarios (envs/doom_games.py).
//
// ONE thread per env runs the whole agent step: `frameskip` physics sub-frames,
// reward / done / episode return, the auto-reset of finished envs, and the scene
// (the per-env rectangle list in painter's order, int16 y0/x0/h/w) that
// rects_stack_push (csrc/preprocess.hip) rasterises, converts to gray, resizes and
// pushes into the frame stack.  So a game step is two launches and no torch ops;
// the torch implementation (atari_games.py) stays the bit-exact oracle
// (tests/test_games_hip.py).
//
// State: int32 [N][NS] per game, one row per env (the kernel keeps the row in
// registers).  Boolean grids are bit-packed (bricks 108 b, aliens 36 b, maze eggs
// 143 b, mushrooms 320 b).  The field order of every game is mirrored by
// `HIP_FIELDS` of its class in envs/atari_games.py.
//
// Integer semantics follow torch: `//` and `%` are floor division / floor modulo,
// the counter-based RNG (env_rand_u32) is shared with envs/base.py.
#include "common.h"

namespace games {

DEVI int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
DEVI int fdiv(int a, int b) {            // python a // b
  const int q = a / b;
  return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}
DEVI int fmodi(int a, int b) {           // python a % b
  const int r = a % b;
  return (r != 0 && ((r < 0) != (b < 0))) ? r + b : r;
}
DEVI int iabs(int v) { return v < 0 ? -v : v; }
DEVI bool getbit(const int* w, int i) { return ((uint32_t)w[i >> 5] >> (i & 31)) & 1u; }
DEVI void setbit(int* w, int i, bool v) {
  const uint32_t m = 1u << (i & 31);
  w[i >> 5] = (int)(v ? ((uint32_t)w[i >> 5] | m) : ((uint32_t)w[i >> 5] & ~m));
}
DEVI void fill_bits(int* w, int nbits) {
  for (int i = 0; i < (nbits + 31) / 32; ++i) {
    const int rem = nbits - 32 * i;
    w[i] = rem >= 32 ? -1 : (int)((1u << rem) - 1u);
  }
}
DEVI bool any_bits(const int* w, int nbits) {
  bool a = false;
  for (int i = 0; i < (nbits + 31) / 32; ++i) a |= w[i] != 0;
  return a;
}

struct Rng {
  uint32_t seed, env, counter;
  DEVI int rand(uint32_t stream, uint32_t n) const { return (int)(env_rand_u32(seed, env, counter, stream) % n); }
};

DEVI void rect(int16_t* r, int i, int y0, int x0, int h, int w) {
  r[4 * i + 0] = (int16_t)clampi(y0, -32768, 32767);
  r[4 * i + 1] = (int16_t)clampi(x0, -32768, 32767);
  r[4 * i + 2] = (int16_t)clampi(h, -32768, 32767);
  r[4 * i + 3] = (int16_t)clampi(w, -32768, 32767);
}

// --------------------------------------------------------------------------- Breakout
struct Breakout {
  static constexpr int U = 16, ROWS = 6, COLS = 18, NB = ROWS * COLS;
  static constexpr int BRICK_Y0 = 57, BRICK_H = 6, BRICK_W = 8, BRICK_X0 = 8, PADDLE_Y = 189, PADDLE_W = 16;
  enum { PX, BX, BY, VX, VY, INPLAY, LIVES, BR, COUNTER = BR + 4, STEPS, EPRET, NS };
  static constexpr int R = 3 + NB + 2;
  static DEVI int row_reward(int r) { return r < 2 ? 7 : (r < 4 ? 4 : 1); }
  static DEVI void reset(int* s, const Rng&) {
    fill_bits(s + BR, NB);
    s[PX] = 72 * U;
    s[INPLAY] = 0;
    s[LIVES] = 5;
  }
  static DEVI int physics(int* s, int a, const Rng& g) {
    const int right = a == 2, left = a == 3;
    s[PX] = clampi(s[PX] + (right - left) * 6 * U, 8 * U, (152 - PADDLE_W) * U);
    bool inplay = s[INPLAY] != 0;
    const bool serve = !inplay && a == 1;
    const int dirn = g.rand(0, 2) == 0 ? -1 : 1;
    if (serve) {
      s[BX] = s[PX] + (PADDLE_W / 2) * U;
      s[BY] = 120 * U;
      s[VX] = dirn * (24 + g.rand(1, 12));
      s[VY] = 40;
    }
    inplay = inplay || serve;
    int nx = s[BX] + s[VX], ny = s[BY] + s[VY];
    if ((nx < 8 * U || nx > 150 * U) && inplay) s[VX] = -s[VX];
    nx = clampi(nx, 8 * U, 150 * U);
    const bool hit_top = ny < 32 * U;
    if (hit_top && inplay) s[VY] = iabs(s[VY]);
    if (hit_top) ny = 32 * U;
    const int cy = fdiv(fdiv(ny, U) - BRICK_Y0, BRICK_H), cx = fdiv(fdiv(nx, U) - BRICK_X0, BRICK_W);
    const bool inb = cy >= 0 && cy < ROWS && cx >= 0 && cx < COLS && inplay;
    const int cyc = clampi(cy, 0, ROWS - 1), cxc = clampi(cx, 0, COLS - 1);
    const bool b = getbit(s + BR, cyc * COLS + cxc);
    const bool hitb = inb && b;
    const int reward = hitb ? row_reward(cyc) : 0;
    setbit(s + BR, cyc * COLS + cxc, b && !hitb);
    if (hitb) s[VY] = -s[VY];
    const int nyu = fdiv(ny, U);
    const bool onp = s[VY] > 0 && nyu >= PADDLE_Y - 4 && nyu < PADDLE_Y + 2 && nx >= s[PX] - 2 * U &&
                     nx <= s[PX] + (PADDLE_W + 2) * U;
    const int off = nx - (s[PX] + (PADDLE_W / 2) * U);
    if (onp && inplay) {
      s[VX] = clampi(fdiv(off * 3, 16), -48, 48);
      s[VY] = -iabs(s[VY]);
    }
    const bool lost = inplay && ny > 200 * U;
    s[LIVES] -= lost;
    inplay = inplay && !lost;
    if (inplay) {
      s[BX] = nx;
      s[BY] = ny;
    }
    s[INPLAY] = inplay;
    return reward;
  }
  static DEVI bool over(const int* s) { return s[LIVES] <= 0 || !any_bits(s + BR, NB); }
  static DEVI void scene(const int* s, int16_t* r) {
    rect(r, 0, 17, 0, 15, 160);
    rect(r, 1, 17, 0, 179, 8);
    rect(r, 2, 17, 152, 179, 8);
    for (int i = 0; i < NB; ++i)
      rect(r, 3 + i, BRICK_Y0 + (i / COLS) * BRICK_H, BRICK_X0 + (i % COLS) * BRICK_W, getbit(s + BR, i) ? BRICK_H : 0,
           BRICK_W);
    rect(r, 3 + NB, PADDLE_Y, fdiv(s[PX], U), 4, PADDLE_W);
    rect(r, 4 + NB, fdiv(s[BY], U), fdiv(s[BX], U), s[INPLAY] ? 4 : 0, 2);
  }
};

// --------------------------------------------------------------------------- SpaceInvaders
struct SpaceInvaders {
  static constexpr int AR = 6, AC = 6;
  enum { FX, FY, FDIR, TICK, PX, LIVES, SX, SY, SHOT, BXP, BYP, BOMB, ALIVE, COUNTER = ALIVE + 2, STEPS, EPRET, NS };
  static constexpr int R = 1 + AR * AC + 3;
  static DEVI void reset(int* s, const Rng&) {
    fill_bits(s + ALIVE, AR * AC);
    s[FX] = 22;
    s[FY] = 40;
    s[FDIR] = 1;
    s[TICK] = 0;
    s[PX] = 76;
    s[LIVES] = 3;
    s[SHOT] = 0;
    s[BOMB] = 0;
  }
  static DEVI bool alive(const int* s, int r, int c) { return getbit(s + ALIVE, r * AC + c); }
  static DEVI int physics(int* s, int a, const Rng& g) {
    const int right = a == 2 || a == 4, left = a == 3 || a == 5;
    const bool fire = a == 1 || a == 4 || a == 5;
    s[PX] = clampi(s[PX] + 2 * (right - left), 20, 133);
    bool shot = s[SHOT] != 0;
    const bool new_shot = fire && !shot;
    if (new_shot) {
      s[SX] = s[PX] + 3;
      s[SY] = 182;
    }
    shot = shot || new_shot;
    s[SY] -= 4 * shot;
    shot = shot && s[SY] > 20;
    // formation march every 4 sub-frames (column occupancy taken BEFORE this sub-frame's hit, as the oracle)
    s[TICK] += 1;
    const bool move = fmodi(s[TICK], 4) == 0;
    int cols = 0;
    for (int c = 0; c < AC; ++c)
      for (int r = 0; r < AR; ++r) cols |= (alive(s, r, c) ? 1 : 0) << c;
    int leftmost = AC, rightmost = -1;
    for (int c = AC - 1; c >= 0; --c)
      if ((cols >> c) & 1) leftmost = c;
    for (int c = 0; c < AC; ++c)
      if ((cols >> c) & 1) rightmost = c;
    const int xl = s[FX] + 16 * leftmost, xr = s[FX] + 16 * rightmost + 8;
    const bool edge = move && ((s[FDIR] > 0 && xr >= 150) || (s[FDIR] < 0 && xl <= 10));
    if (edge) s[FDIR] = -s[FDIR];
    s[FY] += 4 * edge;
    if (move && !edge) s[FX] += s[FDIR];
    // shot vs aliens
    const int col = fdiv(s[SX] - s[FX], 16), row = fdiv(s[SY] - s[FY], 18);
    const bool inx = fmodi(s[SX] - s[FX], 16) < 8, iny = fmodi(s[SY] - s[FY], 18) < 10;
    const bool ok = shot && col >= 0 && col < AC && row >= 0 && row < AR && inx && iny;
    const int colc = clampi(col, 0, AC - 1), rowc = clampi(row, 0, AR - 1);
    const bool al = alive(s, rowc, colc);
    const bool hit = ok && al;
    setbit(s + ALIVE, rowc * AC + colc, al && !hit);
    const int reward = hit ? 30 - 5 * rowc : 0;
    shot = shot && !hit;
    // alien bomb
    bool bomb = s[BOMB] != 0;
    bool drop = !bomb && g.rand(4, 64) == 0 && cols != 0;
    const int bc = g.rand(5, AC);
    const bool has = (cols >> bc) & 1;
    int lowest = -1;
    for (int r = 0; r < AR; ++r)
      if (alive(s, r, bc)) lowest = r;
    drop = drop && has;
    if (drop) {
      s[BXP] = s[FX] + 16 * bc + 4;
      s[BYP] = s[FY] + 18 * lowest + 10;
    }
    bomb = bomb || drop;
    s[BYP] += 2 * bomb;
    const bool hitp = bomb && s[BYP] >= 185 && s[BYP] < 193 && s[BXP] >= s[PX] && s[BXP] < s[PX] + 7;
    s[LIVES] -= hitp;
    s[BOMB] = bomb && !hitp && s[BYP] < 196;
    s[SHOT] = shot;
    if (!any_bits(s + ALIVE, AR * AC)) {      // wave cleared: a new formation marches in from the top
      fill_bits(s + ALIVE, AR * AC);
      s[FX] = 22;
      s[FY] = 40;
      s[FDIR] = 1;
    }
    return reward;
  }
  static DEVI bool over(const int* s) {
    int lowest_row = -1;
    for (int r = 0; r < AR; ++r)
      for (int c = 0; c < AC; ++c)
        if (alive(s, r, c)) lowest_row = r;
    const bool invaded = s[FY] + 18 * lowest_row + 10 >= 180;
    return s[LIVES] <= 0 || invaded;
  }
  static DEVI void scene(const int* s, int16_t* r) {
    rect(r, 0, 195, 0, 2, 160);
    for (int i = 0; i < AR * AC; ++i)
      rect(r, 1 + i, s[FY] + 18 * (i / AC), s[FX] + 16 * (i % AC), getbit(s + ALIVE, i) ? 10 : 0, 8);
    rect(r, 1 + AR * AC, 185, s[PX], 8, 7);
    rect(r, 2 + AR * AC, s[SY], s[SX], s[SHOT] ? 6 : 0, 1);
    rect(r, 3 + AR * AC, s[BYP], s[BXP], s[BOMB] ? 6 : 0, 1);
  }
};

// --------------------------------------------------------------------------- Alien / MsPacman
// 13 x 11 maze (envs/atari_games.py MAZE): bit x of row y set = wall
__constant__ int MAZE_ROWS[11] = {0x1FFF, 0x1041, 0x175D, 0x1001, 0x15F5, 0x1445, 0x175D, 0x1001, 0x175D, 0x1041, 0x1FFF};
struct AlienBase {
  static constexpr int H = 11, W = 13, NA = 3, CW = 12, CH = 16, Y0 = 20, X0 = 2, NWALL = 77;
  enum { PY, PX, AY, AX = AY + NA, LIVES = AX + NA, TICK, DOTS, COUNTER = DOTS + 5, STEPS, EPRET, NS };
  static constexpr int R = NWALL + H * W + 1 + NA;
  static DEVI bool wall(int y, int x) { return (MAZE_ROWS[clampi(y, 0, H - 1)] >> clampi(x, 0, W - 1)) & 1; }
  static DEVI int dy(int j) { return j == 1 ? -1 : (j == 4 ? 1 : 0); }       // none, up, right, left, down
  static DEVI int dx(int j) { return j == 2 ? 1 : (j == 3 ? -1 : 0); }
  static DEVI int amap(int a) {
    const int m[18] = {0, 0, 1, 2, 3, 4, 1, 1, 4, 4, 1, 2, 3, 4, 1, 1, 4, 4};
    return m[a];
  }
  static DEVI void start(int k, int& y, int& x) {
    y = k == 2 ? 9 : 1;
    x = k == 0 ? 1 : (k == 1 ? 11 : 6);
  }
  static DEVI void reset(int* s, const Rng&) {
    for (int i = 0; i < 5; ++i) s[DOTS + i] = 0;
    for (int i = 0; i < H * W; ++i) setbit(s + DOTS, i, !wall(i / W, i % W));
    s[PY] = 7;
    s[PX] = 6;
    setbit(s + DOTS, 7 * W + 6, false);
    for (int k = 0; k < NA; ++k) start(k, s[AY + k], s[AX + k]);
    s[LIVES] = 3;
    s[TICK] = 0;
  }
  static DEVI int physics(int* s, int a, const Rng& g) {
    s[TICK] += 1;
    const bool step_now = fmodi(s[TICK], 2) == 0;
    const int di = amap(a);
    const int ny = s[PY] + dy(di), nx = s[PX] + dx(di);
    if (step_now && !wall(ny, nx)) {
      s[PY] = ny;
      s[PX] = nx;
    }
    const int cell = s[PY] * W + s[PX];
    int reward = getbit(s + DOTS, cell) ? 10 : 0;
    setbit(s + DOTS, cell, false);
    const bool amove = fmodi(s[TICK], 4) == 0;
    for (int k = 0; k < NA; ++k) {
      const int y = s[AY + k], x = s[AX + k];
      int by = y, bx = x, bd = 1 << 20;
      const int r = g.rand(6 + k, 4);
      for (int j = 1; j < 5; ++j) {
        const int cy = y + dy(j), cx = x + dx(j);
        int d = iabs(cy - s[PY]) + iabs(cx - s[PX]);
        if (r == j - 1) d -= 2;
        if (!wall(cy, cx) && d < bd) {
          by = cy;
          bx = cx;
          bd = d;
        }
      }
      if (amove) {
        s[AY + k] = by;
        s[AX + k] = bx;
      }
    }
    bool caught = false;
    for (int k = 0; k < NA; ++k) caught |= s[AY + k] == s[PY] && s[AX + k] == s[PX];
    s[LIVES] -= caught;
    if (caught)
      for (int k = 0; k < NA; ++k) start(k, s[AY + k], s[AX + k]);
    if (!any_bits(s + DOTS, H * W)) reward += 500;
    return reward;
  }
  static DEVI bool over(const int* s) { return s[LIVES] <= 0 || !any_bits(s + DOTS, H * W); }
  static DEVI void scene(const int* s, int16_t* r) {
    int n = 0;
    for (int i = 0; i < H * W; ++i)
      if (wall(i / W, i % W)) rect(r, n++, Y0 + (i / W) * CH, X0 + (i % W) * CW, CH, CW);
    for (int i = 0; i < H * W; ++i)
      rect(r, NWALL + i, Y0 + (i / W) * CH + CH / 2, X0 + (i % W) * CW + CW / 2, getbit(s + DOTS, i) ? 2 : 0, 2);
    rect(r, NWALL + H * W, Y0 + s[PY] * CH + 3, X0 + s[PX] * CW + 3, 10, 6);
    for (int k = 0; k < NA; ++k) rect(r, NWALL + H * W + 1 + k, Y0 + s[AY + k] * CH + 2, X0 + s[AX + k] * CW + 2, 12, 8);
  }
};
struct Alien : AlienBase {};
struct MsPacman : AlienBase {};

// --------------------------------------------------------------------------- Centipede
struct Centipede {
  static constexpr int NSEG = 10, GH = 20, GW = 16;
  enum { MUSH, SY = MUSH + 10, SX = SY + NSEG, SDIR = SX + NSEG, SALIVE = SDIR + NSEG, PX, SHOT, SHX, SHY, LIVES, TICK,
         COUNTER, STEPS, EPRET, NS };
  static constexpr int R = GH * GW + NSEG + 2;
  static DEVI int amap_h(int a) {
    const int m[18] = {0, 0, 0, 1, -1, 0, 1, -1, 1, -1, 0, 0, 1, -1, 0, 1, -1, 1};
    return m[a];
  }
  static DEVI bool afire(int a) { return a == 1 || a >= 10; }
  static DEVI bool salive(const int* s, int k) { return (s[SALIVE] >> k) & 1; }
  static DEVI void reset(int* s, const Rng& g) {
    for (int i = 0; i < 10; ++i) s[MUSH + i] = 0;
    for (int k = 0; k < GH * GW / 16; ++k) {
      const int r = g.rand(10 + k, 100);
      const int pos = min(k * 16 + r % 16, GH * GW - 1);
      if (pos < (GH - 3) * GW) setbit(s + MUSH, pos, r < 60);
    }
    for (int k = 0; k < NSEG; ++k) {
      s[SY + k] = 0;
      s[SX + k] = max(GW - 1 - k, 0);
      s[SDIR + k] = -1;
    }
    s[SALIVE] = (1 << NSEG) - 1;
    s[PX] = 76;
    s[SHOT] = 0;
    s[LIVES] = 3;
    s[TICK] = 0;
  }
  static DEVI int physics(int* s, int a, const Rng&) {
    s[PX] = clampi(s[PX] + 2 * amap_h(a), 4, 152);
    bool shot = s[SHOT] != 0;
    const bool fire = afire(a) && !shot;
    if (fire) {
      s[SHX] = s[PX] + 2;
      s[SHY] = 180;
    }
    shot = shot || fire;
    s[SHY] -= 6 * shot;
    shot = shot && s[SHY] > 20;
    const int gy = clampi(fdiv(s[SHY] - 20, 8), 0, GH - 1), gx = clampi(fdiv(s[SHX], 10), 0, GW - 1);
    const int cell = gy * GW + gx;
    const bool m0 = getbit(s + MUSH, cell);
    const bool hm = shot && m0;
    setbit(s + MUSH, cell, m0 && !hm);
    int reward = hm;
    shot = shot && !hm;
    int hits = 0, alive = s[SALIVE];
    for (int k = 0; k < NSEG; ++k) {
      const bool hs = shot && ((alive >> k) & 1) && s[SY + k] == gy && s[SX + k] == gx;
      hits += hs;
      if (hs) alive &= ~(1 << k);
    }
    reward += 10 * hits;
    s[SALIVE] = alive;
    if (hits) setbit(s + MUSH, cell, true);
    shot = shot && hits == 0;
    s[TICK] += 1;
    const bool tick3 = fmodi(s[TICK], 3) == 0;
    for (int k = 0; k < NSEG; ++k) {
      const bool mv = tick3 && salive(s, k);
      const int nx = s[SX + k] + s[SDIR + k];
      const bool blocked = nx < 0 || nx >= GW || getbit(s + MUSH, s[SY + k] * GW + clampi(nx, 0, GW - 1));
      if (mv && blocked) {
        s[SY + k] = min(s[SY + k] + 1, GH - 1);
        s[SDIR + k] = -s[SDIR + k];
      }
      if (mv && !blocked) s[SX + k] = nx;
    }
    bool reach = false;
    for (int k = 0; k < NSEG; ++k) reach |= salive(s, k) && s[SY + k] >= GH - 1;
    s[LIVES] -= reach;
    if (reach)
      for (int k = 0; k < NSEG; ++k) {
        s[SY + k] = 0;
        s[SX + k] = max(GW - 1 - k, 0);
        s[SDIR + k] = -1;
      }
    if (s[SALIVE] == 0) {
      s[SALIVE] = (1 << NSEG) - 1;
      for (int k = 0; k < NSEG; ++k) s[SY + k] = 0;
    }
    s[SHOT] = shot;
    return reward;
  }
  static DEVI bool over(const int* s) { return s[LIVES] <= 0; }
  static DEVI void scene(const int* s, int16_t* r) {
    for (int i = 0; i < GH * GW; ++i)
      rect(r, i, 20 + (i / GW) * 8, (i % GW) * 10, getbit(s + MUSH, i) ? 8 : 0, 10);
    for (int k = 0; k < NSEG; ++k)
      rect(r, GH * GW + k, 20 + s[SY + k] * 8 + 1, s[SX + k] * 10 + 1, salive(s, k) ? 6 : 0, 8);
    rect(r, GH * GW + NSEG, 184, s[PX], 8, 4);
    rect(r, GH * GW + NSEG + 1, s[SHY], s[SHX], s[SHOT] ? 6 : 0, 1);
  }
};

// --------------------------------------------------------------------------- synthetic Doom scenarios
// envs/doom_games.py: one physics() call is one Doom tic; a finished episode plays no further tic of its agent
// step.  LIVING / DEATH_PENALTY / TIMEOUT are the scenario table's values (envs/doom/scenarios.py; the torch class
// imports them, tests/test_doom_games.py compares them with these).  Per-monster / per-fireball loops run over
// compile-time bounds and never index the state row with a run-time value, so the row stays in registers.
struct DoomView {
  static constexpr int K = 64, Z0 = 32, ZFAR = 96, HORIZON = 80, FH = 50, HUD_Y0 = 186;
  static constexpr int WALL_Y0 = HORIZON - FH * K / (ZFAR + Z0), WALL_H = 2 * (FH * K / (ZFAR + Z0));
  static constexpr int NBACK = 3;
  static DEVI void backdrop(int16_t* r) {
    rect(r, 0, 0, 0, HORIZON, 160);
    rect(r, 1, HORIZON, 0, HUD_Y0 - HORIZON, 160);
    rect(r, 2, WALL_Y0, 0, WALL_H, 160);
  }
  // object of world size w x h on the floor at lateral offset dx (screen x centre cx given), depth z
  static DEVI void object(int16_t* r, int i, int cx, int z, int w, int h, bool visible, int lift = 0) {
    const int den = z + Z0;
    const int pw = fdiv(w * K, den), ph = fdiv(h * K, den);
    const int yb = HORIZON + fdiv(FH * K, den);
    rect(r, i, yb - ph - lift, cx - fdiv(pw, 2), visible ? ph : 0, pw);
  }
  static DEVI int xproj(int dx, int z) { return 80 + fdiv(dx * K, z + Z0); }
  // side-wall edges at +-room and two far-wall pillars at +-pillar, drawn at x - px: rectangles i .. i + 3
  static DEVI void strafe_walls(int16_t* r, int i, int px, int room, int pillar) {
    rect(r, i, WALL_Y0, xproj(-room - px, ZFAR) - 200, WALL_H, 200);
    rect(r, i + 1, WALL_Y0, xproj(room - px, ZFAR), WALL_H, 200);
    object(r, i + 2, xproj(-pillar - px, ZFAR), ZFAR, 8, 2 * FH, true);
    object(r, i + 3, xproj(pillar - px, ZFAR), ZFAR, 8, 2 * FH, true);
  }
  // [gun], HUD strip, health bar, [ammo bar]: returns the next free rectangle
  static DEVI int hud(int16_t* r, int i, int health, int ammo, bool weapon) {
    if (weapon) rect(r, i++, HUD_Y0 - 20, 74, 20, 12);
    rect(r, i++, HUD_Y0, 0, 210 - HUD_Y0, 160);
    rect(r, i++, HUD_Y0 + 4, 8, 6, fdiv(max(health, 0) * 3, 5));
    if (weapon) rect(r, i++, HUD_Y0 + 14, 8, 6, max(ammo, 0) * 2);
    return i;
  }
};

struct DoomBasic : DoomView {
  static constexpr int LIVING = -10, TIMEOUT = 350;
  static constexpr int XMAX = 100, ROOM = 130, SPEED = 4, PILLAR = 50, MON_W = 24, MON_H = 40, MON_HALF = 12;
  static constexpr int KILL = 101, SHOT = -5, COOLDOWN = 8, AMMO = 50;
  enum { PX, MX, COOL, TIC, KILLED, AMMOF, COUNTER, STEPS, EPRET, NS };
  static constexpr int R = NBACK + 4 + 1 + 4;
  static DEVI void reset(int* s, const Rng& g) {
    s[PX] = 0;
    s[MX] = g.rand(20, 2 * XMAX + 1) - XMAX;
    s[COOL] = 0;
    s[TIC] = 0;
    s[AMMOF] = AMMO;
    s[KILLED] = 0;
  }
  static DEVI bool over(const int* s) { return s[KILLED] != 0 || s[TIC] >= TIMEOUT; }
  static DEVI int physics(int* s, int a, const Rng&) {
    if (over(s)) return 0;
    s[TIC] += 1;
    s[PX] = clampi(s[PX] + SPEED * ((a == 2) - (a == 3)), -XMAX, XMAX);
    const int cool = max(s[COOL] - 1, 0);
    const bool fire = a == 1 && cool == 0 && s[AMMOF] > 0;
    const bool hit = fire && iabs(s[MX] - s[PX]) <= MON_HALF;
    s[COOL] = fire ? COOLDOWN : cool;
    s[AMMOF] -= fire;
    s[KILLED] = hit;
    return LIVING + (fire ? SHOT : 0) + (hit ? KILL : 0);
  }
  static DEVI void scene(const int* s, int16_t* r) {
    backdrop(r);
    strafe_walls(r, NBACK, s[PX], ROOM, PILLAR);
    object(r, NBACK + 4, xproj(s[MX] - s[PX], ZFAR), ZFAR, MON_W, MON_H, s[KILLED] == 0);
    hud(r, NBACK + 5, 100, s[AMMOF], true);
  }
};

struct DoomDefendCenter : DoomView {
  static constexpr int DEATH_PENALTY = 1, TIMEOUT = 2100;
  static constexpr int NM = 5, NP = 8, TURN = 3, DMAX = 96, STAGGER = 8, MON_W = 16, MON_H = 40;
  static constexpr int TOL0 = 6, TOLDIV = 8, COOLDOWN = 8, AMMO = 26, RESPAWN = 16, BITE = 8, DAMAGE = 10, HEALTH = 100;
  enum { TH, COOL, AMMOF, HEALTHF, TIC, MA, MD = MA + NM, MT = MD + NM, ALIVE = MT + NM, COUNTER, STEPS, EPRET, NS };
  static constexpr int R = NBACK + NP + NM + 4;
  static DEVI int spawn_angle(const Rng& g, int k, int tic) { return fmodi(g.rand(30 + k, 256) + tic * 41, 256); }
  static DEVI int offset(int ang, int th) { return fmodi(ang - th + 128, 256) - 128; }
  static DEVI void reset(int* s, const Rng& g) {
    s[TH] = 0;
    s[COOL] = 0;
    s[AMMOF] = AMMO;
    s[HEALTHF] = HEALTH;
    s[TIC] = 0;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      s[MA + k] = spawn_angle(g, k, 0);
      s[MD + k] = DMAX - STAGGER * k;
      s[MT + k] = 0;
    }
    s[ALIVE] = (1 << NM) - 1;
  }
  static DEVI bool over(const int* s) {
    return s[HEALTHF] <= 0 || s[TIC] >= TIMEOUT || (s[AMMOF] <= 0 && s[COOL] <= 0);
  }
  static DEVI int physics(int* s, int a, const Rng& g) {
    if (over(s)) return 0;
    s[TIC] += 1;
    s[TH] = fmodi(s[TH] + TURN * ((a == 2) - (a == 3)), 256);
    const int cool = max(s[COOL] - 1, 0);
    const bool fire = a == 1 && cool == 0 && s[AMMOF] > 0;
    s[COOL] = fire ? COOLDOWN : cool;
    s[AMMOF] -= fire;
    int alive = s[ALIVE];
    // the shot kills the nearest living monster inside its aim tolerance (ties: the lowest index)
    constexpr int BIG = 1 << 20;
    int key = BIG;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      const int tol = TOL0 + fdiv(DMAX - s[MD + k], TOLDIV);
      const bool cand = ((alive >> k) & 1) && iabs(offset(s[MA + k], s[TH])) <= tol;
      key = min(key, cand ? s[MD + k] * 8 + k : BIG);
    }
    const bool kill = fire && key < BIG;
    int reward = kill;
    int biting = 0;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      if (kill && (key & 7) == k) {
        alive &= ~(1 << k);
        s[MT + k] = RESPAWN;
      }
      if ((alive >> k) & 1) {                    // walk inward, bite at distance 0
        s[MD + k] = max(s[MD + k] - 1, 0);
        biting += s[MD + k] == 0;
      }
    }
    if (fmodi(s[TIC], BITE) == 0) s[HEALTHF] -= biting * DAMAGE;
#pragma unroll
    for (int k = 0; k < NM; ++k)                 // dead slots come back at the rim after RESPAWN tics
      if (!((alive >> k) & 1)) {
        s[MT + k] = max(s[MT + k] - 1, 0);
        if (s[MT + k] == 0) {
          alive |= 1 << k;
          s[MD + k] = DMAX;
          s[MA + k] = spawn_angle(g, k, s[TIC]);
        }
      }
    s[ALIVE] = alive;
    if (s[HEALTHF] <= 0) reward -= DEATH_PENALTY;
    return reward;
  }
  static DEVI void scene(const int* s, int16_t* r) {
    backdrop(r);
#pragma unroll
    for (int k = 0; k < NP; ++k) object(r, NBACK + k, 80 + fdiv(offset(32 * k, s[TH]) * 5, 2), ZFAR, 8, 2 * FH, true);
#pragma unroll
    for (int k = 0; k < NM; ++k)
      object(r, NBACK + NP + k, 80 + fdiv(offset(s[MA + k], s[TH]) * 5, 2), s[MD + k], MON_W, MON_H,
             (s[ALIVE] >> k) & 1);
    hud(r, NBACK + NP + NM, s[HEALTHF], s[AMMOF], true);
  }
};

struct DoomTakeCover : DoomView {
  static constexpr int LIVING = 1, TIMEOUT = 2100;
  static constexpr int XMAX = 100, ROOM = 130, SPEED = 4, PILLAR = 50, NSH = 6, NF = 6, SH_W = 16, SH_H = 40;
  static constexpr int GROW = 200, FIRE = 8, U = 16, FSPEED = 8, FB_W = 12, FB_H = 12, FB_LIFT = 25;
  static constexpr int HIT_W = 12, DAMAGE = 20, HEALTH = 100;
  enum { PX, HEALTHF, TIC, FX, FZ = FX + NF, FVX = FZ + NF, FACT = FVX + NF, COUNTER, STEPS, EPRET, NS };
  static constexpr int R = NBACK + 4 + NSH + NF + 2;
  static DEVI int shooter_x(int j) {           // in the order the shooters appear
    return j == 0 ? -18 : j == 1 ? 54 : j == 2 ? -90 : j == 3 ? 90 : j == 4 ? -54 : 18;
  }
  static DEVI int shooters(const int* s) { return min(1 + fdiv(s[TIC], GROW), NSH); }
  static DEVI void reset(int* s, const Rng&) {
    s[PX] = 0;
    s[HEALTHF] = HEALTH;
    s[TIC] = 0;
    s[FACT] = 0;
  }
  static DEVI bool over(const int* s) { return s[HEALTHF] <= 0 || s[TIC] >= TIMEOUT; }
  static DEVI int physics(int* s, int a, const Rng& g) {
    if (over(s)) return 0;
    s[TIC] += 1;
    s[PX] = clampi(s[PX] + SPEED * ((a == 1) - (a == 2)), -XMAX, XMAX);
    int act = s[FACT], hits = 0;
#pragma unroll
    for (int k = 0; k < NF; ++k)                 // fireballs in flight
      if ((act >> k) & 1) {
        s[FZ + k] -= FSPEED;
        s[FX + k] += s[FVX + k];
        if (s[FZ + k] <= 0) {
          hits += iabs(fdiv(s[FX + k], U) - s[PX]) <= HIT_W;
          act &= ~(1 << k);
        }
      }
    int idle = NF;                               // the lowest idle slot after the arrivals
#pragma unroll
    for (int k = NF - 1; k >= 0; --k)
      if (!((act >> k) & 1)) idle = k;
    s[HEALTHF] -= DAMAGE * hits;
    // thrown at where the player stands now (selects on the values: a branch per slot made the compiler pick the
    // slot by address, which put the fireball fields in scratch)
    const bool launch = fmodi(s[TIC], FIRE) == 0 && idle < NF;
    const int sx = shooter_x(fmodi(g.rand(40, NSH) + fdiv(s[TIC], FIRE), shooters(s)));
    const int vx = fdiv((s[PX] - sx) * U, ZFAR / FSPEED);
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const bool here = launch && k == idle;
      s[FX + k] = here ? sx * U : s[FX + k];
      s[FZ + k] = here ? ZFAR : s[FZ + k];
      s[FVX + k] = here ? vx : s[FVX + k];
      act |= (here ? 1 : 0) << k;
    }
    s[FACT] = act;
    return LIVING;
  }
  static DEVI void scene(const int* s, int16_t* r) {
    backdrop(r);
    strafe_walls(r, NBACK, s[PX], ROOM, PILLAR);
    const int ns = shooters(s);
#pragma unroll
    for (int j = 0; j < NSH; ++j)
      object(r, NBACK + 4 + j, xproj(shooter_x(j) - s[PX], ZFAR), ZFAR, SH_W, SH_H, j < ns);
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const int z = max(s[FZ + k], 0);
      object(r, NBACK + 4 + NSH + k, xproj(fdiv(s[FX + k], U) - s[PX], z), z, FB_W, FB_H, (s[FACT] >> k) & 1,
             fdiv(FB_LIFT * K, z + Z0));
    }
    hud(r, NBACK + 4 + NSH + NF, s[HEALTHF], 0, false);
  }
};

// --------------------------------------------------------------------------- free-view Doom scenarios
// A player with a position (px, pz) in 1/U world units and a heading th (256 units a turn, 0 looks along +z,
// positive turns right) in a room: DoomDefendLine, DoomHealthGathering, DoomCorridor (envs/doom_games.py,
// DoomNavVec).  Integer only: isin / icos come from the quarter-wave table QSIN[i] = round(256 sin(2 pi i / 256)).
//
// Painter's order without sorting: every rectangle slot has a fixed colour, objects that can overlap each other share
// one colour, and the kinds are layered by an argument that holds in every frame.  Posts stand on the walls of a
// convex room (the far line, the square room's walls, the corridor's side walls), so whatever inside the room
// overlaps a post on screen is nearer than it: backdrop, posts, vest, enemies or kits, fireballs, HUD.  (Fireballs
// are painted over every monster, as in DoomTakeCover: a glowing ball is seen through a nearer monster.)
__constant__ int QSIN[65] = {0, 6, 13, 19, 25, 31, 38, 44, 50, 56, 62, 68, 74, 80, 86, 92, 98, 104, 109, 115, 121, 126,
                             132, 137, 142, 147, 152, 157, 162, 167, 172, 177, 181, 185, 190, 194, 198, 202, 206, 209,
                             213, 216, 220, 223, 226, 229, 231, 234, 237, 239, 241, 243, 245, 247, 248, 250, 251, 252,
                             253, 254, 255, 255, 256, 256, 256};

struct DoomNav : DoomView {
  static constexpr int U = 16, ZVIEW = 160, COL = 80, DXMAX = 512;
  static constexpr int BIG = 1 << 20;
  struct V { int dx, dz; };
  static DEVI int isin(int h) {
    h = fmodi(h, 256);
    const int k = h & 127;
    const int q = QSIN[k <= 64 ? k : 128 - k];
    return h >= 128 ? -q : q;
  }
  static DEVI int icos(int h) { return isin(h + 64); }
  // view offset in whole world units of (rx, rz), given in 1/div units, for sn = isin(th), cs = icos(th).
  // int32 bound: |rx|, |rz| <= 2^14 (DoomCorridor: 1000 * 16 sub-units) and |sn|, |cs| <= 2^8, so each product is at
  // most 2^22 and their sum at most 2^23.
  static DEVI V view(int rx, int rz, int sn, int cs, int div) {
    return {fdiv(rx * cs - rz * sn, 256 * div), fdiv(rx * sn + rz * cs, 256 * div)};
  }
  static DEVI bool drawn(V v) { return v.dz >= 0 && v.dz <= ZVIEW; }
  // the hit-scan rule: the object's drawn rectangle covers the sights' column
  static DEVI bool covers(V v, int w) {
    const int den = clampi(v.dz, 0, ZVIEW) + Z0;
    const int pw = fdiv(w * K, den);
    const int x0 = 80 + fdiv(clampi(v.dx, -DXMAX, DXMAX) * K, den) - fdiv(pw, 2);
    return drawn(v) && x0 <= COL && COL < x0 + pw;
  }
  static DEVI void nav_object(int16_t* r, int i, V v, int w, int h, bool visible, int lift = 0) {
    const int z = clampi(v.dz, 0, ZVIEW);
    object(r, i, 80 + fdiv(clampi(v.dx, -DXMAX, DXMAX) * K, z + Z0), z, w, h, visible && drawn(v),
           fdiv(lift * K, z + Z0));
  }
};

struct DoomDefendLine : DoomNav {
  static constexpr int DEATH_PENALTY = 1, TIMEOUT = 2100;
  static constexpr int NM = 6, NF = 3, NP = 5, TURN = 2, TH_MAX = 40, DMAX = 96, STAGGER = 32, STANDOFF = 48;
  static constexpr int MON_W = 24, MON_H = 40, SH_W = 20, SH_H = 48, POST_W = 12, POST_GAP = 48;
  static constexpr int COOLDOWN = 8, RESPAWN = 16, HP_MAX = 3, BITE = 8, DAMAGE = 10, HEALTH = 100;
  static constexpr int FIRE = 24, FPHASE = 8, FSPEED = 4, FDAMAGE = 6, FB_W = 12, FB_H = 12, FB_LIFT = 25;
  enum { TH, COOL, HEALTHF, TIC, MD, MHP = MD + NM, MT = MHP + NM, MK = MT + NM, FD = MK + NM, ALIVE = FD + NF, FACT,
         COUNTER, STEPS, EPRET, NS };
  static constexpr int R = NBACK + NP + NM + NF + 3;
  static DEVI int lane_x(int k) { return -100 + 40 * k; }      // LANE_X
  static DEVI V monster(const int* s, int k, int sn, int cs) {
    return view(fdiv(lane_x(k) * s[MD + k], DMAX), s[MD + k], sn, cs, 1);
  }
  static DEVI void reset(int* s, const Rng& g) {
    s[TH] = 0;
    s[COOL] = 0;
    s[HEALTHF] = HEALTH;
    s[TIC] = 0;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      s[MD + k] = DMAX - g.rand(80 + k, STAGGER);
      s[MHP + k] = 1;
      s[MT + k] = 0;
      s[MK + k] = 0;
    }
#pragma unroll
    for (int j = 0; j < NF; ++j) s[FD + j] = 0;
    s[ALIVE] = (1 << NM) - 1;
    s[FACT] = 0;
  }
  static DEVI bool over(const int* s) { return s[HEALTHF] <= 0 || s[TIC] >= TIMEOUT; }
  static DEVI int physics(int* s, int a, const Rng&) {
    if (over(s)) return 0;
    s[TIC] += 1;
    s[TH] = clampi(s[TH] + TURN * ((a == 2) - (a == 3)), -TH_MAX, TH_MAX);
    const int cool = max(s[COOL] - 1, 0);
    const bool fire = a == 1 && cool == 0;
    s[COOL] = fire ? COOLDOWN : cool;
    const int sn = isin(s[TH]), cs = icos(s[TH]);
    int alive = s[ALIVE], act = s[FACT];
    int key = BIG;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      const V v = monster(s, k, sn, cs);
      const bool cand = ((alive >> k) & 1) && covers(v, (k & 1) ? SH_W : MON_W);
      key = min(key, cand ? v.dz * 8 + k : BIG);
    }
    const bool hit = fire && key < BIG;
    int reward = 0, biting = 0;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      const bool shot = hit && (key & 7) == k;
      s[MHP + k] -= shot;
      const bool dead = shot && s[MHP + k] <= 0;
      alive &= ~((dead ? 1 : 0) << k);
      s[MT + k] = dead ? RESPAWN : s[MT + k];
      s[MK + k] += dead;
      reward += dead;
      if ((alive >> k) & 1) {                    // melee walk to the player, shooters to their stand-off
        s[MD + k] = max(s[MD + k] - 1, (k & 1) ? STANDOFF : 0);
        biting += !(k & 1) && s[MD + k] == 0;
      }
    }
    if (fmodi(s[TIC], BITE) == 0) s[HEALTHF] -= biting * DAMAGE;
#pragma unroll
    for (int j = 0; j < NF; ++j) {               // fireball j belongs to shooter 2 j + 1
      const int k = 2 * j + 1;
      if ((act >> j) & 1) {
        s[FD + j] -= FSPEED;
        if (s[FD + j] <= 0) {
          s[HEALTHF] -= FDAMAGE;
          act &= ~(1 << j);
        }
      }
      const bool launch = ((alive >> k) & 1) && s[MD + k] == STANDOFF && !((act >> j) & 1) &&
                          fmodi(s[TIC] + FPHASE * j, FIRE) == 0;
      s[FD + j] = launch ? STANDOFF : s[FD + j];
      act |= (launch ? 1 : 0) << j;
    }
#pragma unroll
    for (int k = 0; k < NM; ++k)                 // dead slots come back at the far line, tougher
      if (!((alive >> k) & 1)) {
        s[MT + k] = max(s[MT + k] - 1, 0);
        if (s[MT + k] == 0) {
          alive |= 1 << k;
          s[MD + k] = DMAX;
          s[MHP + k] = min(1 + s[MK + k], HP_MAX);
        }
      }
    s[ALIVE] = alive;
    s[FACT] = act;
    if (s[HEALTHF] <= 0) reward -= DEATH_PENALTY;
    return reward;
  }
  static DEVI void scene(const int* s, int16_t* r) {
    backdrop(r);
    const int sn = isin(s[TH]), cs = icos(s[TH]);
#pragma unroll
    for (int k = 0; k < NP; ++k)
      nav_object(r, NBACK + k, view((k - NP / 2) * POST_GAP, DMAX, sn, cs, 1), POST_W, 2 * FH, true);
#pragma unroll
    for (int k = 0; k < NM; ++k)
      nav_object(r, NBACK + NP + k, monster(s, k, sn, cs), (k & 1) ? SH_W : MON_W, (k & 1) ? SH_H : MON_H,
                 (s[ALIVE] >> k) & 1);
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const int fd = max(s[FD + j], 0);
      nav_object(r, NBACK + NP + NM + j, view(fdiv(lane_x(2 * j + 1) * fd, DMAX), fd, sn, cs, 1), FB_W, FB_H,
                 (s[FACT] >> j) & 1, FB_LIFT);
    }
    rect(r, NBACK + NP + NM + NF, HUD_Y0 - 20, 74, 20, 12);      // the gun; unlimited ammo has no bar
    hud(r, NBACK + NP + NM + NF + 1, s[HEALTHF], 0, false);
  }
};

struct DoomHealthGathering : DoomNav {
  static constexpr int LIVING = 1, DEATH_PENALTY = 100, TIMEOUT = 2100;
  static constexpr int NK = 8, KIT0 = 4, NP = 8, ROOM = 96, KROOM = 88, SPEED = 4, TURN = 4;
  static constexpr int ACID = 16, ACID_DMG = 8, SPAWN = 32, PICK = 12, HEAL = 25, HMAX = 100, HEALTH = 100;
  static constexpr int KIT_W = 12, KIT_H = 12, POST_W = 12, KMULX = 37, KMULZ = 59;
  enum { PX, PZ, TH, HEALTHF, TIC, KX, KZ = KX + NK, KACT = KZ + NK, COUNTER, STEPS, EPRET, NS };
  static constexpr int R = NBACK + NP + NK + 2;
  static constexpr int SPAN = 2 * KROOM + 1;
  // corners and wall middles, clockwise from (-ROOM, -ROOM)
  static DEVI int post_x(int k) { return (k == 0 || k >= 6) ? -ROOM : (k == 1 || k == 5) ? 0 : ROOM; }
  static DEVI int post_z(int k) { return k <= 2 ? -ROOM : (k == 3 || k == 7) ? 0 : ROOM; }
  static DEVI void reset(int* s, const Rng& g) {
    s[PX] = 0;
    s[PZ] = 0;
    s[TH] = g.rand(72, 256);
    s[HEALTHF] = HEALTH;
    s[TIC] = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      s[KX + k] = k < KIT0 ? g.rand(50 + k, SPAN) - KROOM : 0;
      s[KZ + k] = k < KIT0 ? g.rand(60 + k, SPAN) - KROOM : 0;
    }
    s[KACT] = (1 << KIT0) - 1;
  }
  static DEVI bool over(const int* s) { return s[HEALTHF] <= 0 || s[TIC] >= TIMEOUT; }
  static DEVI int physics(int* s, int a, const Rng& g) {
    if (over(s)) return 0;
    s[TIC] += 1;
    s[TH] = fmodi(s[TH] + TURN * ((a == 2) - (a == 3)), 256);
    const int fwd = a == 1 ? SPEED * U : 0;
    s[PX] = clampi(s[PX] + fdiv(fwd * isin(s[TH]), 256), -ROOM * U, ROOM * U);
    s[PZ] = clampi(s[PZ] + fdiv(fwd * icos(s[TH]), 256), -ROOM * U, ROOM * U);
    const int wx = fdiv(s[PX], U), wz = fdiv(s[PZ], U);
    int act = s[KACT], picked = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const bool pick = ((act >> k) & 1) && iabs(s[KX + k] - wx) <= PICK && iabs(s[KZ + k] - wz) <= PICK;
      picked += pick;
      act &= ~((pick ? 1 : 0) << k);
    }
    if (picked) s[HEALTHF] = min(s[HEALTHF] + HEAL * picked, HMAX);
    if (fmodi(s[TIC], ACID) == 0) s[HEALTHF] -= ACID_DMG;
    int empty = NK;                              // a new kit into the lowest empty slot
#pragma unroll
    for (int k = NK - 1; k >= 0; --k)
      if (!((act >> k) & 1)) empty = k;
    const bool spawn = fmodi(s[TIC], SPAWN) == 0;
    const int nx = fmodi(g.rand(70, SPAN) + s[TIC] * KMULX, SPAN) - KROOM;
    const int nz = fmodi(g.rand(71, SPAN) + s[TIC] * KMULZ, SPAN) - KROOM;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const bool here = spawn && k == empty;
      s[KX + k] = here ? nx : s[KX + k];
      s[KZ + k] = here ? nz : s[KZ + k];
      act |= (here ? 1 : 0) << k;
    }
    s[KACT] = act;
    return LIVING - (s[HEALTHF] <= 0 ? DEATH_PENALTY : 0);
  }
  static DEVI void scene(const int* s, int16_t* r) {
    backdrop(r);
    const int sn = isin(s[TH]), cs = icos(s[TH]);
#pragma unroll
    for (int k = 0; k < NP; ++k)
      nav_object(r, NBACK + k, view(post_x(k) * U - s[PX], post_z(k) * U - s[PZ], sn, cs, U), POST_W, 2 * FH, true);
#pragma unroll
    for (int k = 0; k < NK; ++k)
      nav_object(r, NBACK + NP + k, view(s[KX + k] * U - s[PX], s[KZ + k] * U - s[PZ], sn, cs, U), KIT_W, KIT_H,
                 (s[KACT] >> k) & 1);
    hud(r, NBACK + NP + NK, s[HEALTHF], 0, false);
  }
};

struct DoomCorridor : DoomNav {
  static constexpr int DEATH_PENALTY = 100, TIMEOUT = 2100;
  static constexpr int NE = 6, NPOST = 5, HALFW = 56, LEN = 1000, SPEED = 4, TURN = 2;
  static constexpr int ENEMY_X = 40, EN_W = 24, EN_H = 40, RANGE = 160, EFIRE = 20, EPHASE = 3, EDMG = 8, EMISS = 4;
  static constexpr int COOLDOWN = 8, AMMO = 26, HEALTH = 100, TOUCH = 24;
  static constexpr int POST_W = 12, POST_GAP = 40, VEST_W = 16, VEST_H = 16;
  enum { PX, PZ, TH, HEALTHF, AMMOF, COOL, TIC, WON, ALIVE, COUNTER, STEPS, EPRET, NS };
  static constexpr int R = NBACK + 2 * NPOST + 1 + NE + 4;
  static DEVI int enemy_x(int i) { return (i & 1) ? ENEMY_X : -ENEMY_X; }
  static DEVI int enemy_z(int i) { return i < 2 ? 250 : i < 4 ? 500 : 750; }      // GROUP_Z
  static DEVI V enemy(const int* s, int i, int sn, int cs) {
    return view(enemy_x(i) * U - s[PX], enemy_z(i) * U - s[PZ], sn, cs, U);
  }
  static DEVI void reset(int* s, const Rng&) {
    s[PX] = 0;
    s[PZ] = 0;
    s[TH] = 0;
    s[HEALTHF] = HEALTH;
    s[AMMOF] = AMMO;
    s[COOL] = 0;
    s[TIC] = 0;
    s[WON] = 0;
    s[ALIVE] = (1 << NE) - 1;
  }
  static DEVI bool over(const int* s) { return s[WON] != 0 || s[HEALTHF] <= 0 || s[TIC] >= TIMEOUT; }
  static DEVI int physics(int* s, int a, const Rng& g) {
    if (over(s)) return 0;
    s[TIC] += 1;
    s[TH] = fmodi(s[TH] + TURN * ((a == 5) - (a == 6)), 256);
    const int fwd = a == 4, side = (a == 2) - (a == 3);
    const int sn = isin(s[TH]), cs = icos(s[TH]);
    const int old = fdiv(s[PZ], U);
    s[PX] = clampi(s[PX] + fdiv(SPEED * U * (fwd * sn + side * cs), 256), -HALFW * U, HALFW * U);
    s[PZ] = clampi(s[PZ] + fdiv(SPEED * U * (fwd * cs - side * sn), 256), 0, LEN * U);
    const int wx = fdiv(s[PX], U), wz = fdiv(s[PZ], U);
    int reward = wz - old;                       // whole-unit progress towards the vest
    const int cool = max(s[COOL] - 1, 0);
    const bool fire = a == 1 && cool == 0 && s[AMMOF] > 0;
    s[COOL] = fire ? COOLDOWN : cool;
    s[AMMOF] -= fire;
    int alive = s[ALIVE];
    int key = BIG;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const V v = enemy(s, i, sn, cs);
      const bool cand = ((alive >> i) & 1) && covers(v, EN_W);
      key = min(key, cand ? v.dz * 8 + i : BIG);
    }
    if (fire && key < BIG) alive &= ~(1 << (key & 7));
    const int r90 = g.rand(90, EMISS);
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const bool shoot = ((alive >> i) & 1) && iabs(enemy_z(i) - wz) <= RANGE && fmodi(s[TIC] + EPHASE * i, EFIRE) == 0 &&
                         fmodi(r90 + s[TIC] * 41 + i * 3, EMISS) != 0;
      s[HEALTHF] -= shoot ? EDMG : 0;
    }
    s[ALIVE] = alive;
    s[WON] = iabs(wx) <= TOUCH && LEN - wz <= TOUCH;
    if (s[HEALTHF] <= 0) reward -= DEATH_PENALTY;
    return reward;
  }
  static DEVI void scene(const int* s, int16_t* r) {
    backdrop(r);
    const int sn = isin(s[TH]), cs = icos(s[TH]);
    const int base = fdiv(fdiv(s[PZ], U), POST_GAP) - 1;       // the window of posts slides with the player
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
      for (int j = 0; j < NPOST; ++j) {
        const int zj = (base + j) * POST_GAP;
        nav_object(r, NBACK + side * NPOST + j,
                   view((side ? HALFW : -HALFW) * U - s[PX], zj * U - s[PZ], sn, cs, U), POST_W, 2 * FH,
                   zj >= 0 && zj <= LEN);
      }
    nav_object(r, NBACK + 2 * NPOST, view(-s[PX], LEN * U - s[PZ], sn, cs, U), VEST_W, VEST_H, true);
#pragma unroll
    for (int i = 0; i < NE; ++i)
      nav_object(r, NBACK + 2 * NPOST + 1 + i, enemy(s, i, sn, cs), EN_W, EN_H, (s[ALIVE] >> i) & 1);
    hud(r, NBACK + 2 * NPOST + 1 + NE, s[HEALTHF], s[AMMOF], true);
  }
};

// --------------------------------------------------------------------------- the last three Doom levels
// envs/doom_world_games.py: DoomMyWayHome, DoomPredictPosition, DoomDeathmatch.  The living reward of the first two
// (-0.0001 a tic) rounds to 0: rewards are integers.
//
// DoomMyWayHome is the first world that is not convex: free space is the union of NR rectangular regions (rooms, the
// dead-end corridor, one doorway per door).  Only the region the player stands in is drawn, and a region is convex,
// so the painter's order above still holds: door openings (part of the wall's surface), posts, vest.  region_of is the
// integer rule both implementations share.  The region's constants are picked by selects over the unrolled table.
// int32 bound of view(): the map spans 416 x 272 world units = 6656 x 4352 sub-units, below the 2^14 of DoomNav::view.
struct DoomMyWayHome : DoomNav {
  static constexpr int TIMEOUT = 2100;
  static constexpr int NR = 10, NROOMS = 5, NSTART = 4, ND = 4, NP = 8;
  static constexpr int VEST_ROOM = 4, VEST_X = 208, VEST_Z = 208, WALL_T = 16, MARGIN = 16, ROOM_SIZE = 128;
  static constexpr int SPEED = 4, TURN = 4, TOUCH = 16, DOOR_W = 32, DOOR_H = 70, POST_W = 12, VEST_W = 16, VEST_H = 16;
  enum { PX, PZ, TH, TIC, WON, COUNTER, STEPS, EPRET, NS };
  static constexpr int R = NBACK + ND + NP + 1 + 2;
  struct Region { int x0, z0, x1, z1, doors, marks; };
  //                                        A  B    C    D  E    F    AB   BC   AD  DE
  static DEVI Region region(int k) {
    constexpr int X0[NR] = {0, 144, 288, 0, 144, 336, 128, 272, 48, 128};
    constexpr int Z0R[NR] = {0, 0, 0, 144, 144, 128, 48, 48, 128, 192};
    constexpr int X1[NR] = {128, 272, 416, 128, 272, 368, 144, 288, 80, 144};
    constexpr int Z1R[NR] = {128, 128, 128, 272, 272, 272, 80, 80, 144, 224};
    constexpr int DOORS[NR] = {3, 10, 9, 6, 8, 4, 10, 10, 5, 10};
    constexpr int MARKS[NR] = {4, 1, 6, 9, 7, 0, 0, 0, 0, 0};
    return {X0[k], Z0R[k], X1[k], Z1R[k], DOORS[k], MARKS[k]};
  }
  static DEVI int region_of(int px, int pz) {
    int r = -1;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const Region g = region(k);
      r = (px >= g.x0 * U && px < g.x1 * U && pz >= g.z0 * U && pz < g.z1 * U) ? k : r;
    }
    return r;
  }
  static DEVI void reset(int* s, const Rng& g) {
    const int room = g.rand(100, NSTART);
    int x0 = 0, z0 = 0;
#pragma unroll
    for (int k = 0; k < NSTART; ++k) {
      x0 = room == k ? region(k).x0 : x0;
      z0 = room == k ? region(k).z0 : z0;
    }
    s[PX] = (x0 + MARGIN + g.rand(101, ROOM_SIZE - 2 * MARGIN)) * U;
    s[PZ] = (z0 + MARGIN + g.rand(102, ROOM_SIZE - 2 * MARGIN)) * U;
    s[TH] = g.rand(103, 256);
    s[TIC] = 0;
    s[WON] = 0;
  }
  static DEVI bool over(const int* s) { return s[WON] != 0 || s[TIC] >= TIMEOUT; }
  static DEVI int physics(int* s, int a, const Rng&) {
    if (over(s)) return 0;
    s[TIC] += 1;
    s[TH] = fmodi(s[TH] + TURN * ((a == 2) - (a == 3)), 256);
    const int fwd = a == 1 ? SPEED * U : 0;
    const int nx = s[PX] + fdiv(fwd * isin(s[TH]), 256);
    s[PX] = region_of(nx, s[PZ]) >= 0 ? nx : s[PX];
    const int nz = s[PZ] + fdiv(fwd * icos(s[TH]), 256);
    s[PZ] = region_of(s[PX], nz) >= 0 ? nz : s[PZ];
    const bool touch = iabs(fdiv(s[PX], U) - VEST_X) <= TOUCH && iabs(fdiv(s[PZ], U) - VEST_Z) <= TOUCH;
    s[WON] = touch;
    return touch;
  }
  static DEVI void scene(const int* s, int16_t* r) {
    backdrop(r);
    const int sn = isin(s[TH]), cs = icos(s[TH]);
    const int here = max(region_of(s[PX], s[PZ]), 0);
    Region g = region(0);
#pragma unroll
    for (int k = 1; k < NR; ++k) {
      const Region q = region(k);
      const bool in = here == k;
      g = {in ? q.x0 : g.x0, in ? q.z0 : g.z0, in ? q.x1 : g.x1, in ? q.z1 : g.z1, in ? q.doors : g.doors,
           in ? q.marks : g.marks};
    }
    const int xm = fdiv(g.x0 + g.x1, 2), zm = fdiv(g.z0 + g.z1, 2);
    const int xq = g.x0 + fdiv(g.x1 - g.x0, 4), zq = g.z0 + fdiv(g.z1 - g.z0, 4);
#pragma unroll
    for (int j = 0; j < ND; ++j) {               // north (z1), east (x1), south (z0), west (x0)
      const int x = j == 1 ? g.x1 : j == 3 ? g.x0 : xm, z = j == 0 ? g.z1 : j == 2 ? g.z0 : zm;
      nav_object(r, NBACK + j, view(x * U - s[PX], z * U - s[PZ], sn, cs, U), DOOR_W, DOOR_H, (g.doors >> j) & 1);
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {               // the corners, then the marker posts of walls n, e, s, w
      const int x = j < 4 ? ((j == 1 || j == 2) ? g.x1 : g.x0) : (j == 5 ? g.x1 : j == 7 ? g.x0 : xq);
      const int z = j < 4 ? (j >= 2 ? g.z1 : g.z0) : (j == 4 ? g.z1 : j == 6 ? g.z0 : zq);
      nav_object(r, NBACK + ND + j, view(x * U - s[PX], z * U - s[PZ], sn, cs, U), POST_W, 2 * FH,
                 j < 4 || ((g.marks >> (j - 4)) & 1));
    }
    nav_object(r, NBACK + ND + NP, view(VEST_X * U - s[PX], VEST_Z * U - s[PZ], sn, cs, U), VEST_W, VEST_H,
               here == VEST_ROOM);
    hud(r, NBACK + ND + NP + 1, 100, 0, false);
  }
};

struct DoomPredictPosition : DoomNav {
  static constexpr int TIMEOUT = 700;
  static constexpr int NP = 5, TURN = 1, TH_MAX = 40, MZ = 120, WALLZ = 128, XMAX = 96, MSPEED = 2, DIRT = 32;
  static constexpr int LOAD = 48, RSPEED = 8, HIT_W = 12, MON_W = 24, MON_H = 40, POST_W = 12, POST_GAP = 48;
  static constexpr int RK_W = 8, RK_H = 8, RK_LIFT = 25;
  enum { TH, TIC, MX, MDIR, RX, RZ, RTH, RACT, AMMOF, KILLED, COUNTER, STEPS, EPRET, NS };
  static constexpr int R = NBACK + NP + 1 + 1 + 4;
  static DEVI void reset(int* s, const Rng& g) {
    s[TH] = 0;
    s[TIC] = 0;
    s[RX] = 0;
    s[RZ] = 0;
    s[RTH] = 0;
    s[AMMOF] = 1;
    s[MX] = g.rand(111, 2 * XMAX + 1) - XMAX;
    s[MDIR] = g.rand(112, 2) * 2 - 1;
    s[RACT] = 0;
    s[KILLED] = 0;
  }
  static DEVI bool over(const int* s) {
    return s[KILLED] != 0 || (s[AMMOF] <= 0 && s[RACT] == 0) || s[TIC] >= TIMEOUT;
  }
  static DEVI int physics(int* s, int a, const Rng& g) {
    if (over(s)) return 0;
    s[TIC] += 1;
    s[TH] = clampi(s[TH] + TURN * ((a == 2) - (a == 3)), -TH_MAX, TH_MAX);
    int mdir = (fmodi(s[TIC], DIRT) == 0 && g.rand(110, 2) == 1) ? -s[MDIR] : s[MDIR];
    const int nmx = s[MX] + mdir * MSPEED;
    s[MDIR] = iabs(nmx) > XMAX ? -mdir : mdir;
    s[MX] = clampi(nmx, -XMAX, XMAX);
    const bool fire = a == 1 && s[TIC] > LOAD && s[AMMOF] > 0;
    s[AMMOF] -= fire;
    s[RX] = fire ? 0 : s[RX];
    s[RZ] = fire ? 0 : s[RZ];
    s[RTH] = fire ? s[TH] : s[RTH];
    const bool fly = fire || s[RACT] != 0;
    s[RX] += fly ? fdiv(RSPEED * U * isin(s[RTH]), 256) : 0;
    s[RZ] += fly ? fdiv(RSPEED * U * icos(s[RTH]), 256) : 0;
    const bool arrive = fly && fdiv(s[RZ], U) >= MZ;
    const bool hit = arrive && iabs(fdiv(s[RX], U) - s[MX]) <= HIT_W;
    s[RACT] = fly && !arrive;
    s[KILLED] = hit;
    return hit;
  }
  static DEVI void scene(const int* s, int16_t* r) {
    backdrop(r);
    const int sn = isin(s[TH]), cs = icos(s[TH]);
#pragma unroll
    for (int k = 0; k < NP; ++k)
      nav_object(r, NBACK + k, view((k - NP / 2) * POST_GAP * U, WALLZ * U, sn, cs, U), POST_W, 2 * FH, true);
    nav_object(r, NBACK + NP, view(s[MX] * U, MZ * U, sn, cs, U), MON_W, MON_H, s[KILLED] == 0);
    nav_object(r, NBACK + NP + 1, view(s[RX], s[RZ], sn, cs, U), RK_W, RK_H, s[RACT] != 0, RK_LIFT);
    hud(r, NBACK + NP + 2, 100, s[AMMOF], true);
  }
};

struct DoomDeathmatch : DoomNav {
  static constexpr int TIMEOUT = 6300;
  static constexpr int NM = 4, NF = 2, NK = 3, NP = 8, ROOM = 96, KROOM = 88, SPEED = 4, TURN = 4, MSPEED = 1;
  static constexpr int HP = 3, MELEE = 10, STANDOFF = 48, FRANGE = 120, RESPAWN = 32;
  static constexpr int BITE = 8, DAMAGE = 6, FIRE = 32, FPHASE = 16, FT = 24, FDAMAGE = 10, HIT = 12;
  static constexpr int HEALTH = 100, HMAX = 100, HEAL = 25, AMMO = 20, AMMO_MAX = 50, AMMO_BOX = 10;
  static constexpr int PISTOL_DMG = 1, PISTOL_COST = 1, PISTOL_CD = 8, SHOTGUN_DMG = 3, SHOTGUN_COST = 2, SHOTGUN_CD = 16;
  static constexpr int SWITCH = 8, PSPAWN = 64, PPHASE = 16, PICK = 12, KMULX = 37, KMULZ = 59, SMUL = 41;
  static constexpr int MON_W = 24, MON_H = 40, SH_W = 20, SH_H = 48, POST_W = 12;
  static constexpr int KIT_W = 12, KIT_H = 12, BOX_W = 8, BOX_H = 16, SG_W = 24, SG_H = 8;
  static constexpr int FB_W = 12, FB_H = 12, FB_LIFT = 25, GUN_W = 12, GUN2_W = 20;
  enum { PX, PZ, TH, HEALTHF, AMMOF, COOL, SWT, WEAPON, HAS2, TIC, MX, MZ = MX + NM, MHP = MZ + NM, MT = MHP + NM,
         FX = MT + NM, FZ = FX + NF, FVX = FZ + NF, FVZ = FVX + NF, FTF = FVZ + NF, KX = FTF + NF, KZ = KX + NK,
         ALIVE = KZ + NK, FACT, KACT, COUNTER, STEPS, EPRET, NS };
  static constexpr int R = NBACK + NP + NK + NM + NF + 4;
  static constexpr int SPAN = 2 * KROOM + 1, WSPAN = 2 * ROOM + 1;
  static DEVI int post_x(int k) { return (k == 0 || k >= 6) ? -ROOM : (k == 1 || k == 5) ? 0 : ROOM; }
  static DEVI int post_z(int k) { return k <= 2 ? -ROOM : (k == 3 || k == 7) ? 0 : ROOM; }
  // slot k comes in on wall k % 4: north, east, south, west
  static DEVI void spawn(int* s, int k, const Rng& g, int tic) {
    const int c = fmodi(g.rand(120 + k, WSPAN) + tic * SMUL, WSPAN) - ROOM;
    const int w = k & 3;
    s[MX + k] = w == 1 ? ROOM : w == 3 ? -ROOM : c;
    s[MZ + k] = w == 0 ? ROOM : w == 2 ? -ROOM : c;
  }
  static DEVI V monster(const int* s, int k, int sn, int cs) {
    return view(s[MX + k] * U - s[PX], s[MZ + k] * U - s[PZ], sn, cs, U);
  }
  static DEVI void reset(int* s, const Rng& g) {
    s[PX] = 0;
    s[PZ] = 0;
    s[TH] = g.rand(140, 256);
    s[HEALTHF] = HEALTH;
    s[AMMOF] = AMMO;
    s[COOL] = 0;
    s[SWT] = 0;
    s[WEAPON] = 0;
    s[HAS2] = 0;
    s[TIC] = 0;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      spawn(s, k, g, 0);
      s[MHP + k] = HP;
      s[MT + k] = 0;
    }
#pragma unroll
    for (int j = 0; j < NF; ++j) s[FX + j] = s[FZ + j] = s[FVX + j] = s[FVZ + j] = s[FTF + j] = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) s[KX + k] = s[KZ + k] = 0;
    s[ALIVE] = (1 << NM) - 1;
    s[FACT] = 0;
    s[KACT] = 0;
  }
  static DEVI bool over(const int* s) { return s[HEALTHF] <= 0 || s[TIC] >= TIMEOUT; }
  static DEVI int physics(int* s, int a, const Rng& g) {
    if (over(s)) return 0;
    s[TIC] += 1;
    s[TH] = fmodi(s[TH] + TURN * ((a == 5) - (a == 6)), 256);
    const int fwd = a == 4, side = (a == 2) - (a == 3);
    const int sn = isin(s[TH]), cs = icos(s[TH]);
    s[PX] = clampi(s[PX] + fdiv(SPEED * U * (fwd * sn + side * cs), 256), -ROOM * U, ROOM * U);
    s[PZ] = clampi(s[PZ] + fdiv(SPEED * U * (fwd * cs - side * sn), 256), -ROOM * U, ROOM * U);
    const int wx = fdiv(s[PX], U), wz = fdiv(s[PZ], U);
    // weapons
    const int swt = max(s[SWT] - 1, 0);
    const bool change = a == 7 && swt == 0 && s[HAS2] != 0;
    s[SWT] = change ? SWITCH : swt;
    s[WEAPON] = change ? 1 - s[WEAPON] : s[WEAPON];
    const bool shotgun = s[WEAPON] == 1;
    const int cost = shotgun ? SHOTGUN_COST : PISTOL_COST;
    const int cool = max(s[COOL] - 1, 0);
    const bool fire = a == 1 && cool == 0 && s[SWT] == 0 && s[AMMOF] >= cost;
    s[COOL] = fire ? (shotgun ? SHOTGUN_CD : PISTOL_CD) : cool;
    s[AMMOF] -= fire ? cost : 0;
    int alive = s[ALIVE], fact = s[FACT], kact = s[KACT];
    int key = BIG;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      const V v = monster(s, k, sn, cs);
      const bool cand = ((alive >> k) & 1) && covers(v, (k & 1) ? SH_W : MON_W);
      key = min(key, cand ? v.dz * 8 + k : BIG);
    }
    const bool hit = fire && key < BIG;
    int reward = 0, biting = 0;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      const bool shot = hit && (key & 7) == k;
      s[MHP + k] -= shot ? (shotgun ? SHOTGUN_DMG : PISTOL_DMG) : 0;
      const bool dead = shot && s[MHP + k] <= 0;
      alive &= ~((dead ? 1 : 0) << k);
      s[MT + k] = dead ? RESPAWN : s[MT + k];
      reward += dead;
      // walk towards the player down to the stop distance; the melee ones bite there
      const bool walk = (alive >> k) & 1;
      const int ox = wx - s[MX + k], oz = wz - s[MZ + k];
      const bool far = max(iabs(ox), iabs(oz)) > ((k & 1) ? STANDOFF : MELEE);
      s[MX + k] += (walk && far) ? MSPEED * ((ox > 0) - (ox < 0)) : 0;
      s[MZ + k] += (walk && far) ? MSPEED * ((oz > 0) - (oz < 0)) : 0;
      biting += walk && !far && !(k & 1);
    }
    if (fmodi(s[TIC], BITE) == 0) s[HEALTHF] -= biting * DAMAGE;
#pragma unroll
    for (int j = 0; j < NF; ++j) {               // fireball j belongs to thrower 2 j + 1
      const int k = 2 * j + 1;
      const bool fly = (fact >> j) & 1;
      s[FTF + j] -= fly;
      s[FX + j] += fly ? s[FVX + j] : 0;
      s[FZ + j] += fly ? s[FVZ + j] : 0;
      const bool arrive = fly && s[FTF + j] <= 0;
      const bool burn = arrive && iabs(fdiv(s[FX + j], U) - wx) <= HIT && iabs(fdiv(s[FZ + j], U) - wz) <= HIT;
      s[HEALTHF] -= burn ? FDAMAGE : 0;
      fact &= ~((arrive ? 1 : 0) << j);
      const bool near = max(iabs(wx - s[MX + k]), iabs(wz - s[MZ + k])) <= FRANGE;
      const bool launch = ((alive >> k) & 1) && near && !((fact >> j) & 1) && fmodi(s[TIC] + FPHASE * j, FIRE) == 0;
      s[FX + j] = launch ? s[MX + k] * U : s[FX + j];
      s[FZ + j] = launch ? s[MZ + k] * U : s[FZ + j];
      s[FVX + j] = launch ? fdiv(s[PX] - s[MX + k] * U, FT) : s[FVX + j];
      s[FVZ + j] = launch ? fdiv(s[PZ] - s[MZ + k] * U, FT) : s[FVZ + j];
      s[FTF + j] = launch ? FT : s[FTF + j];
      fact |= (launch ? 1 : 0) << j;
    }
    // pickups: medkit, ammunition, shotgun
    bool pick[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      pick[k] = ((kact >> k) & 1) && iabs(s[KX + k] - wx) <= PICK && iabs(s[KZ + k] - wz) <= PICK;
      kact &= ~((pick[k] ? 1 : 0) << k);
    }
    s[HEALTHF] = pick[0] ? min(s[HEALTHF] + HEAL, HMAX) : s[HEALTHF];
    s[AMMOF] = pick[1] ? min(s[AMMOF] + AMMO_BOX, AMMO_MAX) : s[AMMOF];
    s[HAS2] = (s[HAS2] != 0 || pick[2]) ? 1 : 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const bool fresh = fmodi(s[TIC], PSPAWN) == PPHASE * k && !((kact >> k) & 1) && (k != 2 || s[HAS2] == 0);
      s[KX + k] = fresh ? fmodi(g.rand(130 + k, SPAN) + s[TIC] * KMULX, SPAN) - KROOM : s[KX + k];
      s[KZ + k] = fresh ? fmodi(g.rand(133 + k, SPAN) + s[TIC] * KMULZ, SPAN) - KROOM : s[KZ + k];
      kact |= (fresh ? 1 : 0) << k;
    }
#pragma unroll
    for (int k = 0; k < NM; ++k)                 // dead slots come back at their wall
      if (!((alive >> k) & 1)) {
        s[MT + k] = max(s[MT + k] - 1, 0);
        if (s[MT + k] == 0) {
          alive |= 1 << k;
          spawn(s, k, g, s[TIC]);
          s[MHP + k] = HP;
        }
      }
    s[ALIVE] = alive;
    s[FACT] = fact;
    s[KACT] = kact;
    return reward;
  }
  static DEVI void scene(const int* s, int16_t* r) {
    backdrop(r);
    const int sn = isin(s[TH]), cs = icos(s[TH]);
#pragma unroll
    for (int k = 0; k < NP; ++k)
      nav_object(r, NBACK + k, view(post_x(k) * U - s[PX], post_z(k) * U - s[PZ], sn, cs, U), POST_W, 2 * FH, true);
#pragma unroll
    for (int k = 0; k < NK; ++k)
      nav_object(r, NBACK + NP + k, view(s[KX + k] * U - s[PX], s[KZ + k] * U - s[PZ], sn, cs, U),
                 k == 0 ? KIT_W : k == 1 ? BOX_W : SG_W, k == 0 ? KIT_H : k == 1 ? BOX_H : SG_H, (s[KACT] >> k) & 1);
#pragma unroll
    for (int k = 0; k < NM; ++k)
      nav_object(r, NBACK + NP + NK + k, monster(s, k, sn, cs), (k & 1) ? SH_W : MON_W, (k & 1) ? SH_H : MON_H,
                 (s[ALIVE] >> k) & 1);
#pragma unroll
    for (int j = 0; j < NF; ++j)
      nav_object(r, NBACK + NP + NK + NM + j, view(s[FX + j] - s[PX], s[FZ + j] - s[PZ], sn, cs, U), FB_W, FB_H,
                 (s[FACT] >> j) & 1, FB_LIFT);
    const int gw = s[WEAPON] == 1 ? GUN2_W : GUN_W;              // the gun's width shows the weapon in hand
    const int i = NBACK + NP + NK + NM + NF;
    rect(r, i, HUD_Y0 - 20, 80 - fdiv(gw, 2), 20, gw);
    rect(r, i + 1, HUD_Y0, 0, 210 - HUD_Y0, 160);
    rect(r, i + 2, HUD_Y0 + 4, 8, 6, fdiv(max(s[HEALTHF], 0) * 3, 5));
    rect(r, i + 3, HUD_Y0 + 14, 8, 6, max(s[AMMOF], 0) * 2);
  }
};

// --------------------------------------------------------------------------- driver
// mode 0: agent step (actions), mode 1: reset_where(mask).  One thread per env.
template <class G>
__global__ __launch_bounds__(64) void game_step_kernel(int* __restrict__ state, const int* __restrict__ actions,
                                                       const uint8_t* __restrict__ mask, int mode, int n_actions, int N,
                                                       uint32_t seed, uint32_t id_base, int frameskip, int max_steps,
                                                       float* __restrict__ reward, uint8_t* __restrict__ done,
                                                       float* __restrict__ epret, int16_t* __restrict__ rects) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  int s[G::NS];
  int* row = state + (long)e * G::NS;
  for (int i = 0; i < G::NS; ++i) s[i] = row[i];
  Rng g{seed, id_base + (uint32_t)e, (uint32_t)s[G::COUNTER]};   // RNG identity: the global env index
  if (mode == 0) {
    int a = actions[e];
    if (a >= n_actions || a < 0) a = 0;
    int rw = 0;
    for (int f = 0; f < frameskip; ++f) rw += G::physics(s, a, g);
    s[G::COUNTER] += 1;
    s[G::STEPS] += 1;
    s[G::EPRET] += rw;
    const bool d = G::over(s) || s[G::STEPS] >= max_steps;
    reward[e] = (float)rw;
    done[e] = d;
    epret[e] = d ? (float)s[G::EPRET] : 0.f;
    if (d) {
      g.counter = (uint32_t)s[G::COUNTER];
      G::reset(s, g);
      s[G::STEPS] = 0;
      s[G::EPRET] = 0;
      s[G::COUNTER] += 1;
    }
  } else if (mask[e]) {
    G::reset(s, g);
    s[G::STEPS] = 0;
    s[G::EPRET] = 0;
    s[G::COUNTER] += 1;
  }
  for (int i = 0; i < G::NS; ++i) row[i] = s[i];
  G::scene(s, rects + (long)e * G::R * 4);
}

template <class G>
static int launch(void* state, const void* actions, const void* mask, int mode, int n_actions, int N, uint32_t seed,
                  uint32_t id_base, int frameskip, int max_steps, void* reward, void* done, void* epret, void* rects, hipStream_t st) {
  game_step_kernel<G><<<(N + 63) / 64, 64, 0, st>>>((int*)state, (const int*)actions, (const uint8_t*)mask, mode,
                                                    n_actions, N, seed, id_base, frameskip, max_steps, (float*)reward,
                                                    (uint8_t*)done, (float*)epret, (int16_t*)rects);
  return (int)hipGetLastError();
}


// --------------------------------------------------------------------------- meta-Doom
// The nine Doom levels in one batch (envs/doom_meta_games.py is the torch oracle and states the rule).  State row:
// [level state, NSU words | level, unlocked, req, total5, hist[9][5] | counter, steps, epret].  The level state is the
// level's own row without its last three words; words past it are 0.  One thread per env reads `level`, switches to
// the body instantiated from that level's game struct and, at an episode end, scores the episode into the ledger,
// picks the next level and builds its state in a second switch.  Scenes are META_RU rectangles per env (slots past
// the level's R are zeros = hidden); level_out names the level whose scene was written, for the rasteriser's gray
// table.  `table` is int32 [9][4]: lo, target, n_actions, max_steps per level.
constexpr int cmaxi(int a, int b) { return a > b ? a : b; }
template <class G, class... Gs> struct MaxOf {
  static constexpr int NS = cmaxi(G::NS, MaxOf<Gs...>::NS), R = cmaxi(G::R, MaxOf<Gs...>::R);
};
template <class G> struct MaxOf<G> { static constexpr int NS = G::NS, R = G::R; };

struct Meta {
  static constexpr int NL = 9, NH = 5, PASS5 = 3000, FULL5 = 4950, BONUS5 = 2250, RET_MAX = 1000000;
  using Max = MaxOf<DoomBasic, DoomCorridor, DoomDefendCenter, DoomDefendLine, DoomHealthGathering, DoomMyWayHome,
                    DoomPredictPosition, DoomTakeCover, DoomDeathmatch>;
  static constexpr int NSU = Max::NS, RU = Max::R;
  enum { LEVEL = NSU, UNLOCKED, REQ, TOTAL5, HIST, COUNTER = HIST + NL * NH, STEPS, EPRET, NS };
  enum { T_LO, T_TARGET, T_NACT, T_MAXSTEPS, T_COLS };
};

// f(G{}) for the game struct of `level` (0..8, the doom9 order)
template <class F>
DEVI void meta_switch(int level, F&& f) {
  switch (level) {
    case 0: f(DoomBasic{}); break;
    case 1: f(DoomCorridor{}); break;
    case 2: f(DoomDefendCenter{}); break;
    case 3: f(DoomDefendLine{}); break;
    case 4: f(DoomHealthGathering{}); break;
    case 5: f(DoomMyWayHome{}); break;
    case 6: f(DoomPredictPosition{}); break;
    case 7: f(DoomTakeCover{}); break;
    default: f(DoomDeathmatch{}); break;
  }
}

template <class G>
DEVI void meta_load(int* s, const int* row, bool fresh) {
  static_assert(G::COUNTER == G::NS - 3 && G::STEPS == G::NS - 2 && G::EPRET == G::NS - 1, "trailer words");
  for (int i = 0; i < G::NS - 3; ++i) s[i] = fresh ? 0 : row[i];
  s[G::COUNTER] = row[Meta::COUNTER];
  s[G::STEPS] = row[Meta::STEPS];
  s[G::EPRET] = row[Meta::EPRET];
}
template <class G>
DEVI void meta_store(const int* s, int* row) {
  for (int i = 0; i < G::NS - 3; ++i) row[i] = s[i];
  row[Meta::COUNTER] = s[G::COUNTER];
  row[Meta::STEPS] = s[G::STEPS];
  row[Meta::EPRET] = s[G::EPRET];
}
template <class G>
DEVI void meta_scene(const int* s, int16_t* r) {
  G::scene(s, r);
  for (int i = G::R * 4; i < Meta::RU * 4; ++i) r[i] = 0;
}

// The ledger at an episode end (the order of envs/doom_meta_games.py): returns the next level, writes total5.
DEVI int meta_ledger(int* row, const int* __restrict__ table, int level, int ret, int* total5_out) {
  ret = clampi(ret, -Meta::RET_MAX, Meta::RET_MAX);
  const long lo = table[level * Meta::T_COLS + Meta::T_LO];
  const long span = (long)table[level * Meta::T_COLS + Meta::T_TARGET] - lo;
  const long den = span > 0 ? span : 1;
  const long num = 990L * ((long)ret - lo);
  long q = num / den;
  if (num % den != 0 && num < 0) q -= 1;                                   // floor division, den > 0
  const int score = (int)(q < 0 ? 0 : (q > 1000 ? 1000 : q));
  int* h = row + Meta::HIST;
  for (int k = Meta::NH - 1; k > 0; --k) h[level * Meta::NH + k] = h[level * Meta::NH + k - 1];
  h[level * Meta::NH] = score;
  int sums[Meta::NL];
  int total = 0;
  bool all = true;
#pragma unroll
  for (int l = 0; l < Meta::NL; ++l) {
    int v = 0;
#pragma unroll
    for (int k = 0; k < Meta::NH; ++k) v += h[l * Meta::NH + k];
    sums[l] = v;
    total += v;
    all = all && v >= Meta::FULL5;
  }
  int unlocked = row[Meta::UNLOCKED];
#pragma unroll
  for (int i = Meta::NL - 2; i >= 0; --i)
    if (sums[i] >= Meta::PASS5) unlocked |= 1 << (i + 1);
  total += all ? Meta::BONUS5 : 0;
  const int req = row[Meta::REQ];
  int next = 0, best = 0x7FFFFFFF;
#pragma unroll
  for (int l = 0; l < Meta::NL; ++l)
    if (((unlocked >> l) & 1) && sums[l] < best) {
      best = sums[l];
      next = l;
    }
  if (req >= 0 && req < Meta::NL && ((unlocked >> req) & 1)) {
    next = req;
    row[Meta::REQ] = -1;
  }
  row[Meta::UNLOCKED] = unlocked;
  row[Meta::TOTAL5] = total;
  row[Meta::LEVEL] = next;
  *total5_out = total;
  return next;
}

// mode 0: agent step (actions), mode 1: reset_where(mask).  One thread per env, as game_step_kernel.
__global__ __launch_bounds__(64) void meta_step_kernel(int* __restrict__ state, const int* __restrict__ table,
                                                       const int* __restrict__ actions,
                                                       const uint8_t* __restrict__ mask, int mode, int N, uint32_t seed,
                                                       uint32_t id_base, int frameskip, int max_steps,
                                                       float* __restrict__ reward, uint8_t* __restrict__ done,
                                                       float* __restrict__ epret, int16_t* __restrict__ rects,
                                                       uint8_t* __restrict__ level_out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  int* row = state + (long)e * Meta::NS;
  int16_t* sc = rects + (long)e * Meta::RU * 4;
  const uint32_t env = id_base + (uint32_t)e;                              // RNG identity: the global env index
  const int level = clampi(row[Meta::LEVEL], 0, Meta::NL - 1);             // a corrupt word never indexes anything
  int next = level;
  bool enter = false;                                                      // build `next`'s state below
  if (mode == 0) {
    int a = actions[e];
    if (a >= table[level * Meta::T_COLS + Meta::T_NACT] || a < 0) a = 0;
    const int cap = min(table[level * Meta::T_COLS + Meta::T_MAXSTEPS], max_steps);
    int ret = 0;
    meta_switch(level, [&](auto G_) {
      using G = decltype(G_);
      int s[G::NS];
      meta_load<G>(s, row, false);
      Rng g{seed, env, (uint32_t)s[G::COUNTER]};
      int rw = 0;
      for (int f = 0; f < frameskip; ++f) rw += G::physics(s, a, g);
      s[G::COUNTER] += 1;
      s[G::STEPS] += 1;
      s[G::EPRET] += rw;
      enter = G::over(s) || s[G::STEPS] >= cap;
      ret = s[G::EPRET];
      reward[e] = (float)rw;
      meta_store<G>(s, row);
      if (!enter) meta_scene<G>(s, sc);
    });
    done[e] = enter;
    float total = 0.f;
    if (enter) {
      int total5;
      next = meta_ledger(row, table, level, ret, &total5);
      total = (float)total5 * 0.2f;
    }
    epret[e] = total;
  } else {
    enter = mask[e] != 0;
  }
  if (enter || mode != 0)
    meta_switch(next, [&](auto G_) {
      using G = decltype(G_);
      int s[G::NS];
      meta_load<G>(s, row, next != level);
      if (enter) {
        const Rng g{seed, env, (uint32_t)s[G::COUNTER]};
        G::reset(s, g);
        s[G::STEPS] = 0;
        s[G::EPRET] = 0;
        s[G::COUNTER] += 1;
        meta_store<G>(s, row);
        for (int i = G::NS - 3; i < Meta::NSU; ++i) row[i] = 0;
      }
      meta_scene<G>(s, sc);
    });
  level_out[e] = (uint8_t)next;
}

}  // namespace games

// game ids: 0 Breakout, 1 SpaceInvaders, 2 Alien, 3 MsPacman, 4 Centipede, 5 DoomBasic, 6 DoomDefendCenter,
// 7 DoomTakeCover, 8 DoomDefendLine, 9 DoomHealthGathering, 10 DoomCorridor, 12 DoomMyWayHome, 13 DoomPredictPosition,
// 14 DoomDeathmatch.  11 stays unassigned: the launcher's contract names it as the id that no game answers to.
extern "C" int game_layout(int game, int* ns, int* nrects) {
  using namespace games;
  switch (game) {
    case 0: *ns = Breakout::NS; *nrects = Breakout::R; return 0;
    case 1: *ns = SpaceInvaders::NS; *nrects = SpaceInvaders::R; return 0;
    case 2: *ns = Alien::NS; *nrects = Alien::R; return 0;
    case 3: *ns = MsPacman::NS; *nrects = MsPacman::R; return 0;
    case 4: *ns = Centipede::NS; *nrects = Centipede::R; return 0;
    case 5: *ns = DoomBasic::NS; *nrects = DoomBasic::R; return 0;
    case 6: *ns = DoomDefendCenter::NS; *nrects = DoomDefendCenter::R; return 0;
    case 7: *ns = DoomTakeCover::NS; *nrects = DoomTakeCover::R; return 0;
    case 8: *ns = DoomDefendLine::NS; *nrects = DoomDefendLine::R; return 0;
    case 9: *ns = DoomHealthGathering::NS; *nrects = DoomHealthGathering::R; return 0;
    case 10: *ns = DoomCorridor::NS; *nrects = DoomCorridor::R; return 0;
    case 12: *ns = DoomMyWayHome::NS; *nrects = DoomMyWayHome::R; return 0;
    case 13: *ns = DoomPredictPosition::NS; *nrects = DoomPredictPosition::R; return 0;
    case 14: *ns = DoomDeathmatch::NS; *nrects = DoomDeathmatch::R; return 0;
  }
  return -1;
}

extern "C" int launch_game_step(int game, void* state, const void* actions, const void* mask, int mode, int n_actions,
                                int N, uint32_t seed, uint32_t id_base, int frameskip, int max_steps, void* reward, void* done,
                                void* epret, void* rects, hipStream_t st) {
  using namespace games;
  switch (game) {
    case 0: return launch<Breakout>(state, actions, mask, mode, n_actions, N, seed, id_base, frameskip, max_steps, reward, done, epret, rects, st);
    case 1: return launch<SpaceInvaders>(state, actions, mask, mode, n_actions, N, seed, id_base, frameskip, max_steps, reward, done, epret, rects, st);
    case 2: return launch<Alien>(state, actions, mask, mode, n_actions, N, seed, id_base, frameskip, max_steps, reward, done, epret, rects, st);
    case 3: return launch<MsPacman>(state, actions, mask, mode, n_actions, N, seed, id_base, frameskip, max_steps, reward, done, epret, rects, st);
    case 4: return launch<Centipede>(state, actions, mask, mode, n_actions, N, seed, id_base, frameskip, max_steps, reward, done, epret, rects, st);
    case 5: return launch<DoomBasic>(state, actions, mask, mode, n_actions, N, seed, id_base, frameskip, max_steps, reward, done, epret, rects, st);
    case 6: return launch<DoomDefendCenter>(state, actions, mask, mode, n_actions, N, seed, id_base, frameskip, max_steps, reward, done, epret, rects, st);
    case 7: return launch<DoomTakeCover>(state, actions, mask, mode, n_actions, N, seed, id_base, frameskip, max_steps, reward, done, epret, rects, st);
    case 8: return launch<DoomDefendLine>(state, actions, mask, mode, n_actions, N, seed, id_base, frameskip, max_steps, reward, done, epret, rects, st);
    case 9: return launch<DoomHealthGathering>(state, actions, mask, mode, n_actions, N, seed, id_base, frameskip, max_steps, reward, done, epret, rects, st);
    case 10: return launch<DoomCorridor>(state, actions, mask, mode, n_actions, N, seed, id_base, frameskip, max_steps, reward, done, epret, rects, st);
    case 12: return launch<DoomMyWayHome>(state, actions, mask, mode, n_actions, N, seed, id_base, frameskip, max_steps, reward, done, epret, rects, st);
    case 13: return launch<DoomPredictPosition>(state, actions, mask, mode, n_actions, N, seed, id_base, frameskip, max_steps, reward, done, epret, rects, st);
    case 14: return launch<DoomDeathmatch>(state, actions, mask, mode, n_actions, N, seed, id_base, frameskip, max_steps, reward, done, epret, rects, st);
  }
  return -1;
}

// The meta game of the nine Doom levels has entry points of its own (game ids 11 and 15 stay refused above).
extern "C" int meta_layout(int* ns, int* nrects, int* nlevels) {
  if (!ns || !nrects || !nlevels) return -22;
  *ns = games::Meta::NS;
  *nrects = games::Meta::RU;
  *nlevels = games::Meta::NL;
  return 0;
}

extern "C" int launch_meta_step(void* state, const void* table, const void* actions, const void* mask, int mode, int N,
                                uint32_t seed, uint32_t id_base, int frameskip, int max_steps, void* reward, void* done,
                                void* epret, void* rects, void* level_out, hipStream_t st) {
  if (N <= 0 || !state || !table || !rects || !level_out || (mode != 0 && mode != 1)) return -22;
  if (mode == 0 && (!actions || !reward || !done || !epret)) return -22;
  if (mode == 1 && !mask) return -22;
  games::meta_step_kernel<<<(N + 63) / 64, 64, 0, st>>>((int*)state, (const int*)table, (const int*)actions,
                                                        (const uint8_t*)mask, mode, N, seed, id_base, frameskip,
                                                        max_steps, (float*)reward, (uint8_t*)done, (float*)epret,
                                                        (int16_t*)rects, (uint8_t*)level_out);
  return (int)hipGetLastError();
}
