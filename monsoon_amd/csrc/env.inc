// env.inc -- the device-resident vector environment (monsoon_env_reset / monsoon_env_step_dev, include/monsoon.h).
// Included by monsoon_hip.hip inside its anonymous namespace, after the lane-per-game API kernels whose layout it uses
// (ApiEngine, API_LANES, api_load / api_store, attach_rng / lane_commit_rng), so all three record builds get it.  EnvDev
// is in env.h, shared with env_opp.hip (k_env_opp, the heuristic opponent).
//
//   k_env_step    lane per slot: ONE record load for the legality check, the agent's step, the scripted bot's turn, the
//                 end of the episode (winner / fault / truncation, final hash) and, for slots still live, the observation,
//                 legal bytes and to_play (env_finish); one store.  Marks the slots whose episode ended.  With the
//                 heuristic opponent, a slot whose opponent is now to play is put on slot list 0 instead of finished.
//   k_env_opp     (opponent 2) wavefront per listed slot: the opponent's turn (env_opp.hip).
//   k_env_after_opp  (opponent 2) lane per listed slot: env_finish (list 0) or the state views (list 1).
//   k_env_reseed  wavefront per slot (grid n): marked slots only -- the next episode's stream (k_seed's code) and, with a
//                 pool, its decks (k_draw_decks' code).
//   k_env_reseed_schedule  launched in its place by a schedule-mode env: the decks are the pair the handle's deck schedule
//                 draws for the episode's seed (k_draw_schedule's code), then the stream as above.
//   k_env_init    lane per slot, marked slots only: init_game, the bot's opening turn when the agent is SECOND, then the
//                 observation, legal bytes and to_play of the new episode's first state.  With the heuristic opponent, a
//                 new episode that opens with the opponent is put on slot list 1, and k_env_opp / k_env_after_opp follow.
//   k_env_view    lane per (entry, slot) pair of monsoon_env_load_dev, after the copy (k_env_load, env_snap.hip): the views
//                 of every slot that was loaded.
//
// A slot's episode is over when its GameMeta.result is no longer -2 (flags b1 = truncated); k_env_init starts every
// episode with result -2.  Nothing here synchronises with the host: the launches can be captured into a graph.  A
// list's length is cleared by a launch between its last reader and its next writer: list 1's by k_env_step, list 0's by
// k_env_init.

constexpr int ENV_BOT_BOUND = 64;              // bot actions per call before FAULT_BOT_BOUND (a guard, include/monsoon.h)
constexpr uint32_t ENV_POOL_XOR = 0x9E3779B9u;   // the decks' pre-stream (configuration C5, monsoon_draw_decks)

__device__ MSB_INL uint32_t env_seed(const EnvDev& v, int g) { return v.seed0[g] + (uint32_t)v.episode[g] * v.stride; }

// The stream cursor after an engine call that drew from it (as k_step / k_expert commit it), re-attached for the next call.
__device__ MSB_INL void env_commit_rng(ApiEngine& e, const DevBuffers& b, int g, GameMeta& m) {
  if (e.rng_pos() >= (uint32_t)MT_N) e.rng_block_advance();
  lane_commit_rng(b, g, m, e.rng_pos());
  attach_rng(e, b, g, m.rng);
}

__device__ MSB_INL void env_end(GameMeta& m, int result, int fault, bool truncated) {
  m.result = (int8_t)result;
  m.fault = (uint8_t)fault;
  if (truncated) m.flags |= 2;
}

// After a committed step of either side: true when it ended the episode.  A fault first (the reference raises; its step
// returns get_observation(), so an observation that would raise is one too), then a winner (rollout contract, DESIGN.md
// §1), then truncation.
__device__ MSB_INL bool env_after_step(ApiEngine& e, const DevBuffers& b, int g, GameMeta& m, int action, int max_steps) {
  env_commit_rng(e, b, g, m);
  m.steps++;
  m.last_action = (uint8_t)action;
  int f = e.fault();
  if (!f && e.observation_raises()) f = FAULT_INT_CARD;
  if (f) {
    env_end(m, -1, f, false);
  } else if (e.have_winner()) {
    env_end(m, e.winner_of(e.pl_base(0), e.pl_base(1)), 0, false);
    m.flags |= 1;
  } else if (max_steps && m.steps >= max_steps) {
    env_end(m, -1, 0, true);
  }
  return m.result != -2;
}

// The reference's scripted bot (games/stormbound.py:563-637) plays while it is to play: expert_action, then step.
// Returns the steps it committed.
__device__ inline int env_bot_turn(ApiEngine& e, const DevBuffers& b, int g, GameMeta& m, const EnvDev& v) {
  for (int k = 0; k < ENV_BOT_BOUND; k++) {
    if (e.local() == v.agent_side) return k;
    const int a = e.expert_action();
    const int f = e.fault();
    env_commit_rng(e, b, g, m);
    if (f) {   // random.choice([]) inside the bot
      env_end(m, -1, f, false);
      return k;
    }
    e.step(a);
    if (env_after_step(e, b, g, m, a, v.max_steps)) return k + 1;
  }
  if (e.local() != v.agent_side) env_end(m, -1, FAULT_BOT_BOUND, false);
  return ENV_BOT_BOUND;
}

// Puts the calling lanes with on = true on slot list `list`: one atomic per wavefront (same-address atomics serialise at
// ~25 ns each, kernels.h), the lanes' places by rank in the ballot.
__device__ MSB_INL void env_append(const EnvDev& v, int list, int g, bool on) {
  const unsigned long long bal = __ballot(on);
  if (!bal) return;
  const int lane = (int)threadIdx.x & 63;
  const int leader = __builtin_ctzll(bal);
  int base = 0;
  if (lane == leader) base = atomicAdd(&v.opp_count[list * ENV_COUNT_STRIDE], __popcll(bal));
  base = __builtin_amdgcn_readlane(base, leader);
  if (on) v.opp_list[(size_t)list * v.cap + base + __popcll(bal & ((1ull << lane) - 1))] = g;
}

// The views that describe the state slot g is now in: to_play, legal bytes, observation (0 where it raises).
__device__ MSB_INL void env_write_state(ApiEngine& e, const EnvDev& v, int g) {
  if (v.v.to_play) v.v.to_play[g] = (uint8_t)e.local();
  if (v.v.legal) {
    const msb_u64x4 mask = e.legal_mask_v();
    uint32_t* out = (uint32_t*)(v.v.legal + (size_t)g * MONSOON_NUM_ACTIONS);   // 156 = 39 words; 4-byte aligned (checked at reset)
    for (int w = 0; w < MONSOON_NUM_ACTIONS / 4; w++) {
      const uint64_t word = mask[w >> 4];
      const int sh = (4 * w) & 63;
      out[w] = (uint32_t)((word >> sh) & 1) | (uint32_t)((word >> (sh + 1)) & 1) << 8 | (uint32_t)((word >> (sh + 2)) & 1) << 16 |
               (uint32_t)((word >> (sh + 3)) & 1) << 24;
    }
  }
  if (v.v.obs || v.v.obs_raises) {
    const bool r = e.observation_raises();
    if (v.v.obs_raises) v.v.obs_raises[g] = r ? 1 : 0;
    if (v.v.obs) {
      int32_t* out = v.v.obs + (size_t)g * MONSOON_OBS_INTS;
      if (r) {
        for (int i = 0; i < MONSOON_OBS_INTS; i++) out[i] = 0;
      } else {
        e.observe(out);
      }
    }
  }
}

// The end of a step for slot g, whose record is in e and meta in m: the episode count, the end-of-episode views, the
// mark for k_env_reseed / k_env_init, and for a slot still live the views of its state.
__device__ MSB_INL void env_finish(ApiEngine& e, const DevBuffers& b, const EnvDev& v, int g, const GameMeta& m) {
  const bool ended = m.result != -2;
  const int ep = v.episode[g] + (ended ? 1 : 0);
  v.episode[g] = ep;
  v.mark[g] = ended ? 1 : 0;
  v.v.done[g] = ended ? 1 : 0;
  if (v.v.episode) v.v.episode[g] = ep;
  if (v.v.winner) v.v.winner[g] = ended ? m.result : (int8_t)-2;
  if (v.v.truncated) v.v.truncated[g] = (ended && (m.flags & 2)) ? 1 : 0;
  if (v.v.fault) v.v.fault[g] = ended ? m.fault : 0;
  if (v.v.final_hash) {
    uint64_t hsh = 0;
    if (ended) {
      uint8_t rec[CANON_MAX];
      hsh = fnv1a64(rec, canon_record(e, peek_u32(b, g, m.rng), rec));
    }
    v.v.final_hash[g] = hsh;
  }
  if (!ended) env_write_state(e, v, g);
}

__global__ void __launch_bounds__(64) k_env_step(DevBuffers b, EnvDev v, int n, const uint8_t* actions) {
  API_GAME_INDEX();
  if (v.opponent == 2 && g == 0) v.opp_count[ENV_COUNT_STRIDE] = 0;   // list 1: its readers ran in the previous call
  ApiEngine e;
  api_load(b.state + (size_t)g * SW);
  GameMeta m = b.meta[g];
  const int a = actions[g];
  int reward = 0, illegal = 0;
  bool stepped = false, opp_turn = false;
  if (m.result == -2 && a != 255) {   // an episode that ended before the agent could act is reported whatever the action
    const msb_u64x4 mask = e.legal_mask_v();
    const uint64_t word = a < 64 ? mask[0] : (a < 128 ? mask[1] : mask[2]);
    // PASS (155) is always accepted, as k_step accepts it
    if (a >= MONSOON_NUM_ACTIONS || (a != 155 && !((word >> (a & 63)) & 1))) {
      illegal = 1;
    } else {
      attach_rng(e, b, g, m.rng);
      reward = e.step(a) & 1;
      stepped = true;
      const bool ended = env_after_step(e, b, g, m, a, v.max_steps);
      const int bot = (!ended && v.opponent == 1) ? env_bot_turn(e, b, g, m, v) : 0;
      opp_turn = !ended && v.opponent == 2 && e.local() != v.agent_side;   // k_env_opp plays it, k_env_after_opp finishes
      v.agent_steps[g] += 1;
      v.bot_steps[g] += (uint32_t)bot;
    }
  }
  if (v.v.reward) v.v.reward[g] = (int8_t)reward;
  if (v.v.illegal) v.v.illegal[g] = (uint8_t)illegal;
  if (stepped) {
    b.meta[g] = m;
    api_store(b.state + (size_t)g * SW);
  }
  if (v.opponent == 2) env_append(v, 0, g, opp_turn);
  if (!opp_turn) env_finish(e, b, v, g, m);
}

// After k_env_opp: the slots of list `list`, a lane each.  List 0 (the agent's step handed the turn over): env_finish.
// List 1 (a new episode opened with the opponent): the views of the state the opponent left.
__global__ void __launch_bounds__(64) k_env_after_opp(DevBuffers b, EnvDev v, int list) {
  const int count = v.opp_count[list * ENV_COUNT_STRIDE];
  if ((int)blockIdx.x * API_LANES >= count) return;   // uniform: the grid covers n slots, the list is usually short
  lds_init_wtab(b.wk_ovf + (size_t)blockIdx.x * (API_LANES * OVF_WORDS));
  if ((int)threadIdx.x >= API_LANES) return;
  const int i = blockIdx.x * API_LANES + threadIdx.x;
  if (i >= count) return;
  const int g = v.opp_list[(size_t)list * v.cap + i];
  ApiEngine e;
  api_load(b.state + (size_t)g * SW);
  const GameMeta m = b.meta[g];
  attach_rng(e, b, g, m.rng);
  if (list == 0) env_finish(e, b, v, g, m);
  else env_write_state(e, v, g);
}

// k_env_step marked the slots whose episode ended: the next episode's stream and decks.  One wavefront per slot.
__global__ void __launch_bounds__(64) k_env_reseed(DevBuffers b, EnvDev v, int n) {
  __shared__ uint32_t mt[MT_N];
  __shared__ uint32_t words[2 * MT_N];
  __shared__ uint8_t perm[128];
  const int lane = threadIdx.x, g = blockIdx.x;
  if (g >= n || !v.mark[g]) return;
  const uint32_t seed = env_seed(v, g);
  MSB_AS_LDS uint32_t* t = (MSB_AS_LDS uint32_t*)mt;
  if (v.pool_n) {
    // the 1 248 outputs run out for no realistic seed (expected use: 270); k_draw_decks reports it, the env cannot
    (void)wave_draw_decks(seed ^ ENV_POOL_XOR, v.pool, v.pool_n, v.decks + (size_t)g * 24, t, (MSB_AS_LDS uint32_t*)words,
                          (MSB_AS_LDS uint8_t*)perm, lane);
    __syncthreads();
  }
  wave_seed_game(b, g, seed, t, lane);
}

// k_env_reseed for a schedule-mode env: the next episode's decks are the pair that the schedule the handle holds NOW
// (monsoon_env_set_schedule) draws from random.Random(seed32 | generation << 32 | episode seed << 64 | tag << 96), as
// k_draw_schedule draws a game's.  The static LDS is k_draw_schedule's (2 808 bytes, less than k_env_reseed's 7 616): mt
// serves the schedule's stream before wave_seed_game reuses it.  A walk that runs past the 624 outputs cannot fail
// the call (as the pool's cannot): it is counted, and its pair holds card indices of the schedule (the loops of
// deck_schedule.h end on a zero output) but is not the specification's draw.
__global__ void __launch_bounds__(64) k_env_reseed_schedule(DevBuffers b, EnvDev v, int n, EnvSched es) {
  __shared__ uint32_t mt[MT_N];
  __shared__ uint8_t cards[DS_CARD_BYTES];   // archetype[2][12] | pool[2][128]
  __shared__ uint32_t pair[6];
  const int lane = threadIdx.x, g = blockIdx.x;
  if (g >= n || !v.mark[g]) return;
  const uint32_t seed = env_seed(v, g);
  const monsoon_deck_schedule* sc = es.sched;
  const int phase = sc->phase;
  const uint8_t* src = &sc->archetype[0][0];
  for (int k = lane; k < DS_CARD_BYTES; k += 64) cards[k] = src[k];
  if (phase != DS_STATIC) {   // (uniform) the static phase reads no stream
    for (int k = lane; k < MT_N; k += 64) mt[k] = es.mt_init[k];
    __syncthreads();
    if (lane == 0) {
      const uint32_t key[4] = {sc->seed, sc->generation, seed, sc->tag};
      ds_key_mix(mt, key);
    }
    __syncthreads();
    wave_twist_lds((MSB_AS_LDS uint32_t*)mt, lane);
    for (int k = lane; k < MT_N; k += 64) mt[k] = mt_temper(mt[k]);
  }
  __syncthreads();
  if (lane == 0) {
    DsStream s{mt, 0, 0};
    ds_walk(s, phase, sc->n_preserve, sc->balance_archetype_ratio, cards, cards + 24, sc->pool_n, (uint8_t*)pair);
    uint32_t* out = (uint32_t*)(v.decks + (size_t)g * 24);   // 4-byte aligned: d_env's decks start at 16 * cap
    for (int k = 0; k < 6; k++) out[k] = pair[k];
    if (s.over) atomicAdd(es.over, 1u);
  }
  __syncthreads();
  wave_seed_game(b, g, seed, (MSB_AS_LDS uint32_t*)mt, lane);
}

// The first state of the next episode of every marked slot (k_init's code), the bot's opening turn, the slot's views.
// first = 1 (monsoon_env_reset): every slot is marked and the per-call views are cleared too.
__global__ void __launch_bounds__(64) k_env_init(DevBuffers b, EnvDev v, int n, int first) {
  API_GAME_INDEX();
  if (v.opponent == 2 && g == 0) v.opp_count[0] = 0;   // list 0: its readers (k_env_opp, k_env_after_opp) ran before
  if (!v.mark[g]) return;
  ApiEngine e;
  GameMeta m = GameMeta{};   // stream block 0, cursor 0: as k_env_reseed left it
  attach_rng(e, b, g, m.rng);
  const int ep = v.episode[g];
  uint8_t d0[12], d1[12];
  for (int i = 0; i < 12; i++) {
    d0[i] = v.decks[(size_t)g * 24 + i];
    d1[i] = v.decks[(size_t)g * 24 + 12 + i];
  }
  const int f0 = ep == 0 ? v.factions[2 * g] : 0, f1 = ep == 0 ? v.factions[2 * g + 1] : 0;
  e.init_game(d0, d1, f0, f1, env_seed(v, g));
  env_commit_rng(e, b, g, m);
  m.result = -2;
  m.last_action = 255;
  int f = e.fault();
  if (!f && e.observation_raises()) f = FAULT_INT_CARD;   // the reference's reset() returns get_observation()
  bool opp_turn = false;
  if (f) env_end(m, -1, f, false);
  else if (v.opponent == 1 && e.local() != v.agent_side) v.bot_steps[g] += (uint32_t)env_bot_turn(e, b, g, m, v);
  else if (v.opponent == 2) opp_turn = e.local() != v.agent_side;   // the opening turn: k_env_opp on list 1
  b.meta[g] = m;
  api_store(b.state + (size_t)g * SW);
  if (first) {
    v.v.done[g] = 0;
    if (v.v.reward) v.v.reward[g] = 0;
    if (v.v.illegal) v.v.illegal[g] = 0;
    if (v.v.episode) v.v.episode[g] = 0;
    if (v.v.winner) v.v.winner[g] = -2;
    if (v.v.truncated) v.v.truncated[g] = 0;
    if (v.v.fault) v.v.fault[g] = 0;
    if (v.v.final_hash) v.v.final_hash[g] = 0;
  }
  if (v.opponent == 2) env_append(v, 1, g, opp_turn);
  if (!opp_turn) env_write_state(e, v, g);
}

// After k_env_load (env_snap.hip): the views of the slots it loaded, a lane per pair j; dst null = slot j.  They read as
// after a step that ended nothing; for a slot restored with its end pending they are what k_env_init left for it (the
// views of the state the episode ended in: the next step reports the end).  A pair that was skipped writes nothing.
__global__ void __launch_bounds__(64) k_env_view(DevBuffers b, EnvDev v, int m, const int32_t* dst, const uint8_t* loaded) {
  lds_init_wtab(b.wk_ovf + (size_t)blockIdx.x * (API_LANES * OVF_WORDS));
  if ((int)threadIdx.x >= API_LANES) return;
  const int j = blockIdx.x * API_LANES + threadIdx.x;
  if (j >= m || !loaded[j]) return;
  const int g = dst ? dst[j] : j;
  ApiEngine e;
  api_load(b.state + (size_t)g * SW);
  attach_rng(e, b, g, b.meta[g].rng);
  v.mark[g] = 0;
  v.v.done[g] = 0;
  if (v.v.reward) v.v.reward[g] = 0;
  if (v.v.illegal) v.v.illegal[g] = 0;
  if (v.v.episode) v.v.episode[g] = v.episode[g];
  if (v.v.winner) v.v.winner[g] = -2;
  if (v.v.truncated) v.v.truncated[g] = 0;
  if (v.v.fault) v.v.fault[g] = 0;
  if (v.v.final_hash) v.v.final_hash[g] = 0;
  env_write_state(e, v, g);
}
