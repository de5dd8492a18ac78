// replay_log.h -- logged games played again on the device into (observation, action) rows (monsoon_replay_logged_dev,
// include/monsoon.h).  replay_game<U> composes the pieces play_game and after_slot are made of (kernels.h PlayLds<U>,
// legal_set, MSB_EACH_GRANULE, attach_rng, wave_refill; env_after.h obs_word, MSB_OBS_DECK_ORDER): the record is staged in
// column 0 with the stream window attached and stays there; per log entry the wave checks the action against the legal
// set, writes the row of a kept entry, and lane 0 steps column 0 in place -- behind expert_action where the scripted bot
// is to play, which consumes the stream as the rollout did -- before the cursor is committed the way play_game's commit
// does.  No decision is recomputed: no clone, no features, no arg-max; columns 1 .. U-1 stay unused.
// k_replay_log (replay_log.hip) gives every game to one wavefront.
// replay_game<U, true> (monsoon_replay_logged_after_dev, k_replay_after in replay_after.hip) puts after_slot's look-ahead
// (env_after.h MSB_AFTER_STATE) inside it: a kept entry also gets the afterstates of the state its row shows.
#pragma once
#include "env_after.h"

namespace msbk {

// What a launch replays: the batch's part of the log and of the call's row bases, and where its outcome goes.  Game g
// of the batch is match b.meta[g].match of the call.
struct ReplayArgs {
  monsoon_replay_rows rows;   // the caller's columns (all but action may be null)
  const uint8_t* action;      // [n][stride] the logged actions
  const uint8_t* keep;        // [n][stride] non-zero = the entry gets a row; null = every entry
  const int32_t* steps;       // [n] entries of game g
  const int64_t* base;        // [n] the row of game g's first kept entry
  uint8_t* status;            // [n] MONSOON_REPLAY_*
  int32_t* replayed;          // [n] steps committed
  uint8_t* fault;             // [n] meta.fault
  int stride;
};

// Row r: the state column 0 holds, before entry k (action a) of its game is stepped.  Call with the whole wave.
template <int U>
__device__ MSB_INL void replay_row(const DevBuffers& b, const monsoon_replay_rows& o, typename PlayLds<U>::ParEngine& pe, const LegalSet& ls,
                                   const GameMeta& meta, const int g, const size_t r, const int k, const int a, const bool bot, const int lane) {
  typedef PlayLds<U> L;
  if (o.obs || o.obs_raises) {   // (uniform)
    const bool raises = pe.observation_raises();
    if (o.obs) {   // 2 160 bytes: the bulk of a row, in 256-byte stores
      int32_t* out = o.obs + r * MONSOON_OBS_INTS;
      if (raises) {
        for (int i = lane; i < MONSOON_OBS_INTS; i += 64) out[i] = 0;
      } else {
        MSB_AS_LDS uint8_t* ord = (MSB_AS_LDS uint8_t*)(uintptr_t)L::CF;   // (the work stacks are empty between steps)
        MSB_OBS_DECK_ORDER(pe, lane, ord)
        for (int i = lane; i < MONSOON_OBS_INTS; i += 64) out[i] = obs_word(pe, i, ord);
      }
    }
    if (o.obs_raises && lane == 0) o.obs_raises[r] = raises ? 1 : 0;
  }
  if (o.legal && lane < MONSOON_NUM_ACTIONS / 4) {   // 156 bytes = 39 words, a lane each (env.inc env_write_state's layout)
    const uint64_t word = lane < 16 ? ls.mask[0] : (lane < 32 ? ls.mask[1] : ls.mask[2]);
    const int sh = (4 * lane) & 63;
    ((uint32_t*)(o.legal + r * MONSOON_NUM_ACTIONS))[lane] = (uint32_t)((word >> sh) & 1) | (uint32_t)((word >> (sh + 1)) & 1) << 8 |
                                                              (uint32_t)((word >> (sh + 2)) & 1) << 16 | (uint32_t)((word >> (sh + 3)) & 1) << 24;
  }
  if (lane == 0) {
    if (o.to_play) o.to_play[r] = (uint8_t)pe.local();
    o.action[r] = (uint8_t)a;
    if (o.bot) o.bot[r] = bot ? 1 : 0;
    if (o.game) o.game[r] = (int32_t)meta.match;
    if (o.step) o.step[r] = k;
    if (o.state_hash) {   // what monsoon_state_hash reports for this state (k_hash)
      uint8_t rec[CANON_MAX];
      o.state_hash[r] = fnv1a64(rec, canon_record(pe, peek_u32(b, g, meta.rng), rec));
    }
  }
}

// Game g of the batch by the calling wavefront: its log entries, one committed step each.  Call with the whole wave.
// AFTER: every kept entry's row also gets its K afterstates (oa, with the row's rank among the legal actions in chosen).
template <int U, bool AFTER = false>
__device__ MSB_INL void replay_game(const DevBuffers& b, const ReplayArgs& ra, const int g, const int lane,
                                    const monsoon_env_after& oa = monsoon_env_after{}, int16_t* const chosen = nullptr, const int K = 0) {
  typedef PlayLds<U> L;
  GameMeta meta = b.meta[g];
  MSB_AS_LDS u32x4* priv = L::priv();
  u32x4* grec = (u32x4*)(b.state + (size_t)g * SW);
  u32x4 v_rec[L::GPL];   // granules lane, lane + 64, ... of the record: on its way in and out, and across a refill
  _Pragma("unroll") for (int j_ = 0; j_ < L::GPL; j_++) v_rec[j_] = u32x4{0u, 0u, 0u, 0u};
  MSB_EACH_GRANULE(L::GPL, lane, v_rec[j_] = grec[gr_])
  typename L::ParEngine pe;
  typename L::CandEngine ce;   // (lane 0's is column 0 with a work stack)
  // stage: the record in column 0, the stream window attached
  MSB_EACH_GRANULE(L::GPL, lane, *L::gran(0, gr_) = v_rec[j_])
  __syncthreads();
  if (lane == 0) {
    attach_rng(pe, b, g, meta.rng);
    if constexpr (L::COOP_DRAW) *(MSB_AS_LDS uint32_t*)(uintptr_t)DRAW_HINT_LDS = 0u;   // every REPLACE here draws serially, as the bot's do
  }
  __syncthreads();

  const uint8_t* act = ra.action + (size_t)g * ra.stride;
  const uint8_t* keep = ra.keep ? ra.keep + (size_t)g * ra.stride : nullptr;
  const int n_entries = ra.steps[g];
  size_t r = (size_t)ra.base[g];
  int status = MONSOON_REPLAY_OK, done = 0;
  bool over = meta.fault != 0;   // a fault, or an observation that raised after the step before
  for (int k = 0; k < n_entries; k++) {   // (column 0 is the record here)
    if (over || pe.have_winner()) {   // the rollout's end rules
      status = MONSOON_REPLAY_ENDED_EARLY;
      break;
    }
    const int a = act[k];
    const LegalSet ls = legal_set(pe);
    // PASS (155) is always accepted, as k_step accepts it
    const uint64_t word = a < 64 ? ls.mask[0] : (a < 128 ? ls.mask[1] : ls.mask[2]);
    if (a >= MONSOON_NUM_ACTIONS || (a != 155 && !((word >> (a & 63)) & 1))) {
      status = MONSOON_REPLAY_ILLEGAL;
      break;
    }
    const bool bot = (pe.local() == 0 ? meta.p1 : meta.p2) < 0;   // (uniform) the scripted bot is to play
    if (!keep || keep[k]) {
      replay_row<U>(b, ra.rows, pe, ls, meta, g, r, k, a, bot, lane);
      if constexpr (AFTER) {
        // The look-ahead of the row's state.  Its clones overwrite column 0, the live record here: the record (stream window
        // attached) waits in registers and is staged again before lane 0 steps it, so the look-ahead consumes nothing --
        // cursor, stream blocks and meta are the committed ones.  The draw hint it sets is cleared again: the committed
        // REPLACE and the bot draw serially.  (replay_row's order has left the stack area behind the look-ahead's barriers.)
        MSB_EACH_GRANULE(L::GPL, lane, v_rec[j_] = *L::gran(0, gr_))
        if (chosen && lane == 0) {   // the rank of a in the ascending legal list (PASS may be outside it)
          const int rank = __popcll(word & ((1ull << (a & 63)) - 1)) + (a >= 64 ? __popcll(ls.mask[0]) : 0) + (a >= 128 ? __popcll(ls.mask[1]) : 0);
          chosen[r] = (int16_t)(((word >> (a & 63)) & 1) ? rank : -1);
        }
        if (oa.before_features && pe.observation_raises() && lane < 10) oa.before_features[r * 10 + lane] = 0.0;   // (the others: below)
        LegalSet la = ls;
        MSB_AFTER_STATE(oa, K, r, g, meta.rng, la, v_rec, lane)
        meta.lookahead += (uint32_t)(ls.n < K ? ls.n : K);   // the candidates stepped; no decision is counted
        __syncthreads();   // the last pass's successors have been read out of the columns
        MSB_EACH_GRANULE(L::GPL, lane, *L::gran(0, gr_) = v_rec[j_])
        if constexpr (L::COOP_DRAW) {
          if (lane == 0) *(MSB_AS_LDS uint32_t*)(uintptr_t)DRAW_HINT_LDS = 0u;
        }
      }
      r++;
    }
    __syncthreads();   // the row has been read out of column 0 and the order out of the stack area
    int ba = a, f = 0, fs = 0;
    if (lane == 0) {   // (the other lanes wait at the barrier)
      if (bot) {
        ba = ce.expert_action();
        f = ce.fault();   // random.choice([]) inside the bot
      }
      if (!f && ba == a) {
        ce.step(a);
        fs = ce.fault();
        if (!fs && ce.observation_raises()) fs = FAULT_INT_CARD;
      }
    }
    __syncthreads();
    ba = __builtin_amdgcn_readfirstlane(ba);
    f = __builtin_amdgcn_readfirstlane(f);
    fs = __builtin_amdgcn_readfirstlane(fs);
    {   // the commit of play_game: column 0 carries its own cursor; a used-up block is refilled by the whole wave, with the
        // column area as the twist buffer and the record in registers meanwhile
      uint32_t new_pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)pe.rng_pos());
      int cur = (meta.rng >> 16) & 1;
      if (new_pos >= (uint32_t)MT_N) {
        new_pos -= MT_N;
        MSB_EACH_GRANULE(L::GPL, lane, v_rec[j_] = *L::gran(0, gr_))
        __syncthreads();
        wave_refill(b, g, cur, (MSB_AS_LDS uint32_t*)priv, lane);
        MSB_EACH_GRANULE(L::GPL, lane, *L::gran(0, gr_) = v_rec[j_])
        __syncthreads();
        cur ^= 1;
        if (lane == 0) pe.rng_block_advance();
      }
      meta.rng = new_pos | ((uint32_t)cur << 16);
      if (lane == 0) attach_rng(pe, b, g, meta.rng);
      __syncthreads();
    }
    if (f) {   // the bot raised where the log has a step: nothing was stepped
      meta.fault = (uint8_t)f;
      status = MONSOON_REPLAY_BOT_RAISED;
      break;
    }
    if (ba != a) {
      status = MONSOON_REPLAY_BOT_DIFFERS;
      break;
    }
    meta.steps++;
    meta.last_action = (uint8_t)a;
    done++;
    if (fs) {   // a step that faults, or whose observation raises, ends the game
      meta.fault = (uint8_t)fs;
      over = true;
    }
  }
  // the state the game is left in, with the result a rollout would have given it so far
  if (meta.fault) {
    meta.result = -1;
  } else if (pe.have_winner()) {
    meta.result = (int8_t)pe.winner_of(pe.pl_base(0), pe.pl_base(1));
    meta.flags |= 1;
  }
  __syncthreads();
  MSB_EACH_GRANULE(L::GPL, lane, grec[gr_] = *L::gran(0, gr_))
  if (lane == 0) {
    b.meta[g] = meta;
    ra.status[g] = (uint8_t)status;
    ra.replayed[g] = done;
    ra.fault[g] = meta.fault;
  }
}

// k_replay_log<U, W> at the build's default variant (replay_log.hip).
struct ReplayOps : KernelOps {
  void (*launch)(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, ReplayArgs ra, int n, int persistent, int parity);
};
const ReplayOps* monsoon_replay_log_ops();

// k_replay_after<U, W> at the build's default variant (replay_after.hip): k_replay_log with the look-ahead of every kept row.
struct ReplayAfterOps : KernelOps {
  void (*launch)(int grid, int lds_bytes, hipStream_t stream, DevBuffers b, ReplayArgs ra, monsoon_replay_after after, int max_after, int n,
                 int persistent, int parity);
};
const ReplayAfterOps* monsoon_replay_after_ops();

}  // namespace msbk
