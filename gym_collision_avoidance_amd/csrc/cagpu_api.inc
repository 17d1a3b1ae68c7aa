// gym_collision_avoidance_amd/csrc/cagpu_api.inc -- included by cagpu.hip (at file scope, after its anonymous namespace).
// The extern "C" entry points of include/cagpu.h: each checks its arguments, fills its kernel's argument block and hands it
// to the launch layer (csrc/cagpu_launch.inc); no launch is spelled out here except through launch() / launch_lds().
extern "C" {

int cagpu_version(void) { return CAGPU_VERSION; }

const char* cagpu_last_error(void) { return g_err; }

const char* cagpu_last_kernel(void) { return g_last_kernel; }

int cagpu_reset(const CaParams* p, const CaState* s, const CaOut* o, const double* cases, const double* headings,
                const uint8_t* mask, void* stream) {
  int rc = check_params(p, s, o);
  if (rc) return rc;
  if (!cases) return fail(CA_EINVAL, "cagpu_reset: NULL cases%s");
  KArgs k;
  std::memset(&k, 0, sizeof(k));
  k.p = *p; k.s = *s; k.o = *o;
  k.reset_cases = cases; k.reset_headings = headings; k.reset_mask = mask;
  k.n_steps = 1; k.mode = MODE_RESET;
  return launch_any(k, stream);
}

// the argument checks of the map-set entry points (CaMapSet)
static int check_map_set(const CaMapSet* set, const char* who) {
  if (!set || !set->env_map || !set->map.static_bits || set->num_maps < 1)
    return fail(CA_EINVAL, "%s: NULL CaMapSet, env_map or static_bits, or num_maps < 1", who);
  const CaMap& m = set->map;
  if (m.rows < 1 || m.cols < 1 || !(m.cell > 0.0)) return fail(CA_EINVAL, "%s: bad CaMapSet geometry", who);
  return CA_OK;
}

// the argument checks of the policy draw (CaPolicyDraw), shared by cagpu_step_draw and cagpu_policy_draw
// (check_draw_pool: what they reject of d alone -- all cagpu_policy_draw_at, which has no CaAutoReset, can be held to)
static int check_draw_pool(const CaPolicyDraw* d, const char* who) {
  if (!d->cdf || !d->policy_bits) return fail(CA_EINVAL, "%s: NULL CaPolicyDraw.cdf or CaPolicyDraw.policy_bits", who);
  if (d->num_policies < 1 || d->num_policies > 8) return fail(CA_EINVAL, "%s: CaPolicyDraw.num_policies must be in 1..8", who);
  if (d->ensure < -1 || d->ensure >= d->num_policies)
    return fail(CA_EINVAL, "%s: CaPolicyDraw.ensure must be -1 or a pool index below num_policies", who);
  if (d->seed == 0) return fail(CA_EINVAL, "%s: CaPolicyDraw.seed must not be 0", who);
  return CA_OK;
}
static int check_draw(const CaPolicyDraw* d, const CaAutoReset* ar, const char* who) {
  const int rp = check_draw_pool(d, who);
  if (rp) return rp;
  if (!ar) return fail(CA_EINVAL, "%s: a CaPolicyDraw without a CaAutoReset (no table: nothing is ever drawn)", who);
  if (d->seed == ar->heading_seed)
    return fail(CA_EINVAL, "%s: CaPolicyDraw.seed equals CaAutoReset.heading_seed (an agent's heading and policy would be the same uniform)", who);
  return CA_OK;
}

// One step / rollout call as step_impl sees it: the CaStepEx fields plus what only the fixed entry points need.
struct StepCall {
  int32_t n_steps = 1;
  bool ring = false;
  int64_t snapshot_delta = 0;
  const CaMap* map = nullptr;
  const CaMapSet* set = nullptr;
  const CaTraj* traj = nullptr;
  const CaFinal* fin = nullptr;
  const CaEpLog* log = nullptr;
  const CaPolicyDraw* draw = nullptr;  // cagpu_step_draw
  bool maps_multi = false;             // cagpu_step_ex_maps: a map / map set with n_steps > 1 or ring is admitted
  const CaActionTape* tape = nullptr;  // cagpu_step_tape with step_stride != 0 (its `actions` is then the call's `ext`)
  const CaRvoDraw* rd = nullptr;       // cagpu_step_noise
  // the record the entry point insists on (the older names: "traj may not be NULL" ...); cagpu_step_ex: none
  enum Need { NEED_NONE, NEED_SET, NEED_TRAJ, NEED_FIN, NEED_LOG } need = NEED_NONE;
  bool query_snapshot = false;   // cagpu_ring_snapshots: answer 1 / 0 instead of launching
  const char* who = "cagpu";     // the entry point's name in the messages that carry one
};

// the StepCall of a general entry point: what its CaStepEx (NULL: one plain step) and its policy draw spell
static StepCall step_call(const char* who, const CaStepEx* x, const CaPolicyDraw* d = nullptr) {
  StepCall c;
  c.who = who;
  if (x) {
    c.n_steps = x->n_steps; c.ring = x->ring != 0; c.snapshot_delta = x->snapshot_delta;
    c.map = x->map; c.set = x->set; c.traj = x->traj; c.fin = x->fin; c.log = x->log;
  }
  c.draw = d;
  return c;
}

static int step_impl(const CaParams* p, const CaState* s, const CaOut* o, const double* ext, const CaAutoReset* ar,
                     const StepCall& c, void* stream) {
  const CaMapSet* set = c.set;
  const CaTraj* traj = c.traj;
  const CaFinal* fin = c.fin;
  const CaEpLog* log = c.log;
  const int32_t n_steps = c.n_steps;
  const bool want_log = log || c.need == StepCall::NEED_LOG;
  const bool want_fin = fin || c.need == StepCall::NEED_FIN;
  const bool want_traj = traj || c.need == StepCall::NEED_TRAJ;
  if (c.need == StepCall::NEED_SET && !set) return fail(CA_EINVAL, "%s: NULL CaMapSet", c.who);
  if (c.map && set) return fail(CA_EINVAL, "%s: a CaMap and a CaMapSet at once", c.who);
  if (!c.ring && c.snapshot_delta != 0) return fail(CA_EINVAL, "%s: snapshot_delta without ring", c.who);
  if (c.draw) {
    const int rd = check_draw(c.draw, ar, c.who);
    if (rd) return rd;
  }
  if (want_log) {  // (first, like the final record's: a bad episode log is reported as such whatever else is wrong)
    if (!log || !log->rows || !log->head) return fail(CA_EINVAL, "cagpu: NULL CaEpLog, CaEpLog.rows or CaEpLog.head%s");
    if ((reinterpret_cast<uintptr_t>(log->rows) & 15u) || (reinterpret_cast<uintptr_t>(log->head) & 15u))
      return fail(CA_EINVAL, "cagpu: CaEpLog.rows and CaEpLog.head must be 16-byte aligned%s");
    if (log->capacity < 1) return fail(CA_EINVAL, "cagpu: CaEpLog.capacity must be >= 1%s");
    if (!ar) return fail(CA_EINVAL, "cagpu: a CaEpLog without a CaAutoReset (no auto-reset, no episode is ever logged)%s");
  }
  if (want_fin) {  // (first, like the tape's: a bad final record is reported as such whatever else is wrong with the call)
    if (!fin || !fin->obs) return fail(CA_EINVAL, "cagpu: NULL CaFinal or CaFinal.obs%s");
    if ((reinterpret_cast<uintptr_t>(fin->obs) & 15u) || (reinterpret_cast<uintptr_t>(fin->flags) & 3u))
      return fail(CA_EINVAL, "cagpu: CaFinal.obs must be 16-byte aligned (CaFinal.flags: 4-byte)%s");
    if (!ar) return fail(CA_EINVAL, "cagpu: a CaFinal without a CaAutoReset (no auto-reset, nothing is overwritten)%s");
  }
  if (want_traj) {  // (first: a bad tape is reported as such whatever else is wrong with the call)
    if (!traj || !traj->rows) return fail(CA_EINVAL, "cagpu: NULL CaTraj or CaTraj.rows%s");
    if ((reinterpret_cast<uintptr_t>(traj->rows) & 15u) || (reinterpret_cast<uintptr_t>(traj->episode) & 3u))
      return fail(CA_EINVAL, "cagpu: CaTraj.rows must be 16-byte aligned (CaTraj.episode: 4-byte)%s");
  }
  int rc = check_params(p, s, o);
  if (rc) return rc;
  if (set && (rc = check_map_set(set, "cagpu_step_maps"))) return rc;
  if (n_steps < 1) return fail(CA_EINVAL, "cagpu: n_steps must be >= 1%s");
  if ((c.map || set) && (n_steps > 1 || c.ring) && !c.maps_multi)   // (the older names keep refusing: cagpu_step_ex_maps admits it)
    return fail(CA_EINVAL, "%s: a CaMap / CaMapSet with n_steps > 1 or ring (single steps only)", c.who);
  if ((n_steps > 1 || c.ring) && (s->rvo_collab || s->rvo_heading_noise || s->ext_state))
    return fail(CA_EINVAL, "cagpu: CaState.rvo_collab / rvo_heading_noise / ext_state are inputs of ONE step (the caller draws / "
                           "integrates them per step): not accepted by a multi-step call%s");
  KArgs k;
  std::memset(&k, 0, sizeof(k));
  k.p = *p; k.s = *s; k.o = *o; k.ext = ext;
  if (ar) {
    if (!ar->table || ar->n_cases < 1) return fail(CA_EINVAL, "cagpu: bad CaAutoReset%s");
    k.table = ar->table; k.n_cases = ar->n_cases; k.env_id_offset = ar->env_id_offset; k.case_stride = ar->case_stride;
    k.heading_seed = ar->heading_seed;
    k.reset_obs = ar->heading_seed ? nullptr : ar->reset_obs;  // (a reset observation depends on the heading)
    k.reset_plan = ar->heading_seed ? nullptr : ar->reset_plan;
  }
  if (c.map && c.map->static_bits) {
    if (c.map->rows < 1 || c.map->cols < 1 || !(c.map->cell > 0.0)) return fail(CA_EINVAL, "cagpu: bad CaMap%s");
    k.map = *c.map;
  }
  if (set) {
    k.map = set->map;
    k.env_map = set->env_map;
    k.map_words = static_cast<int64_t>(set->map.rows) * ((set->map.cols + 31) / 32);
    k.num_maps = set->num_maps;
    k.map_seed = ar ? set->map_seed : 0;  // (draws happen at auto-resets only)
  }
  k.n_steps = n_steps; k.mode = MODE_STEP;
  if (c.draw) {
    k.draw_cdf = c.draw->cdf; k.draw_bits = c.draw->policy_bits; k.draw_seed = c.draw->seed;
    k.draw_n = c.draw->num_policies; k.draw_ensure = c.draw->ensure;
    k.reset_plan = nullptr;  // (a plan belongs to the policy it was made for: a reset env is queried on its pre-move state)
  }
  if (want_traj) { k.traj_rows = traj->rows; k.traj_ep = traj->episode; }
  if (want_fin) { k.fin_obs = fin->obs; k.fin_flags = fin->flags; }
  if (want_log) {
    k.log_rows = log->rows; k.log_head = log->head; k.log_cap = log->capacity;
    k.log_case_step = static_cast<int32_t>(((k.case_stride % k.n_cases) + k.n_cases) % k.n_cases);
  }
  if (c.tape) {  // (behind every older CA_EINVAL: a call that is wrong in an older way says what it always said)
    const CaActionTape& t = *c.tape;
    if (!t.actions || (reinterpret_cast<uintptr_t>(t.actions) & 15u))
      return fail(CA_EINVAL, "cagpu_step_tape: CaActionTape.actions is NULL or not 16-byte aligned%s");
    if (t.step_stride < 0 || (t.step_stride & 1) || t.step_stride < 2 * static_cast<int64_t>(p->num_envs) * p->num_agents)
      return fail(CA_EINVAL, "cagpu_step_tape: CaActionTape.step_stride must be 0 (one slot held) or even and >= 2 * num_envs * "
                             "num_agents%s");
    k.ext_stride = t.step_stride;
  }
  if (c.rd) {  // (behind the tape's: the RVO draw's rejections are the last CA_EINVAL ones)
    const CaRvoDraw& d = *c.rd;
    if (s->rvo_collab || s->rvo_heading_noise)
      return fail(CA_EINVAL, "cagpu_step_noise: CaState.rvo_collab / rvo_heading_noise beside a CaRvoDraw (one source of these numbers per launch)%s");
    if (d.seed == 0) return fail(CA_EINVAL, "cagpu_step_noise: CaRvoDraw.seed must not be 0%s");
    if ((ar && d.seed == ar->heading_seed) || (c.draw && d.seed == c.draw->seed) || (set && d.seed == set->map_seed))
      return fail(CA_EINVAL, "cagpu_step_noise: CaRvoDraw.seed equals CaAutoReset.heading_seed, CaPolicyDraw.seed or CaMapSet.map_seed "
                             "(two rules would read the same uniforms)%s");
    if (d.collab_coeff < 0.0 && !(d.anti_collab_t > 0.0))
      return fail(CA_EINVAL, "cagpu_step_noise: CaRvoDraw.anti_collab_t must be > 0 with collab_coeff < 0%s");
    if (!(d.noise_std >= 0.0)) return fail(CA_EINVAL, "cagpu_step_noise: CaRvoDraw.noise_std must be >= 0%s");
    if (!(d.collab_coeff < 0.0) && !d.noise_mask)
      return fail(CA_EINVAL, "cagpu_step_noise: both branches of the CaRvoDraw are off (collab_coeff not < 0 and noise_mask NULL)%s");
    if (reinterpret_cast<uintptr_t>(d.address) & 7u)
      return fail(CA_EINVAL, "cagpu_step_noise: CaRvoDraw.address must be 8-byte aligned%s");
    k.rd_seed = d.seed; k.rd_c = d.collab_coeff; k.rd_T = d.anti_collab_t; k.rd_std = d.noise_std;
    k.rd_mask = d.noise_mask; k.rd_addr = d.address;
    k.s.next_action = nullptr;  // (the draw belongs to the query of the step that consumes it: no plan is read or left)
    k.reset_plan = nullptr;
  }
  k.inv_rvo_dt = 1.0 / p->rvo_dt;
  {
    static std::atomic<int> seq{0};
    k.launch_seq = seq.fetch_add(1, std::memory_order_relaxed) + 1;
  }
  if (c.ring) {
    k.ring_agent = static_cast<int64_t>(p->num_envs) * p->num_agents;
    k.ring_obs = k.ring_agent * (6 + 7 * p->max_obs);
    k.ring_env = p->num_envs;
    // the in-kernel snapshot is the pipelined n-step kernel's (launch_pipe with n_steps > 1): every other form of the call
    // leaves it to the caller (cagpu_ring_snapshots says which, from the same arguments)
    const bool can = n_steps > 1 && pipe_eligible(k);
    if (c.query_snapshot) return can ? 1 : 0;
    if (c.snapshot_delta != 0 && !can)
      return fail(CA_EUNSUPPORTED, "cagpu_rollout_ring: snapshot_delta needs the pipelined n-step kernel (cagpu_ring_snapshots() == 1 for these arguments)%s");
    k.snap_delta = c.snapshot_delta;
  }
  return launch_any(k, stream);
}

int cagpu_step_ex(const CaParams* p, const CaState* s, const CaOut* o, const double* ext_actions, const CaAutoReset* ar,
                  const CaStepEx* x, void* stream) {
  return step_impl(p, s, o, ext_actions, ar, step_call("cagpu_step_ex", x), stream);
}

int cagpu_step_draw(const CaParams* p, const CaState* s, const CaOut* o, const double* ext_actions, const CaAutoReset* ar,
                    const CaStepEx* x, const CaPolicyDraw* d, void* stream) {
  if (!d) return cagpu_step_ex(p, s, o, ext_actions, ar, x, stream);
  return step_impl(p, s, o, ext_actions, ar, step_call("cagpu_step_draw", x, d), stream);
}

int cagpu_step_ex_maps(const CaParams* p, const CaState* s, const CaOut* o, const double* ext_actions, const CaAutoReset* ar,
                       const CaStepEx* x, const CaPolicyDraw* d, void* stream) {
  StepCall c = step_call("cagpu_step_ex_maps", x, d);
  c.maps_multi = true;
  return step_impl(p, s, o, ext_actions, ar, c, stream);
}

int cagpu_step_tape(const CaParams* p, const CaState* s, const CaOut* o, const CaActionTape* tape, const CaAutoReset* ar,
                    const CaStepEx* x, const CaPolicyDraw* d, void* stream) {
  // (no tape, or one slot held for all steps: cagpu_step_ex_maps itself)
  if (!tape || tape->step_stride == 0) return cagpu_step_ex_maps(p, s, o, tape ? tape->actions : nullptr, ar, x, d, stream);
  StepCall c = step_call("cagpu_step_ex_maps", x, d);  // (the older rules speak in that entry point's name: same code, same text)
  c.maps_multi = true;
  c.tape = tape;
  return step_impl(p, s, o, tape->actions, ar, c, stream);
}

int cagpu_step_noise(const CaParams* p, const CaState* s, const CaOut* o, const CaActionTape* tape, const CaAutoReset* ar,
                     const CaStepEx* x, const CaPolicyDraw* d, const CaRvoDraw* rd, void* stream) {
  if (!rd) return cagpu_step_tape(p, s, o, tape, ar, x, d, stream);
  StepCall c = step_call("cagpu_step_ex_maps", x, d);  // (the older rules speak in that entry point's name, as for a tape)
  c.maps_multi = true;
  if (tape && tape->step_stride != 0) c.tape = tape;
  c.rd = rd;
  return step_impl(p, s, o, tape ? tape->actions : nullptr, ar, c, stream);
}

int cagpu_rvo_draw_at(const CaRvoDraw* rd, int32_t num_agents, const int64_t* g, const int32_t* k, const int32_t* a,
                      const int32_t* s, int64_t n, uint8_t* out_noncoop_draw, double* out_noise, void* stream) {
  if (!rd || !g || !k || !a || !s || (!out_noncoop_draw && !out_noise) || num_agents < 1 || num_agents > big::NT_MAX || n < 0)
    return fail(CA_EINVAL, "cagpu_rvo_draw_at: NULL pointer, no output, num_agents outside 1..1024 or n < 0%s");
  if (rd->seed == 0) return fail(CA_EINVAL, "cagpu_rvo_draw_at: CaRvoDraw.seed must not be 0%s");
  if (!(rd->noise_std >= 0.0)) return fail(CA_EINVAL, "cagpu_rvo_draw_at: CaRvoDraw.noise_std must be >= 0%s");
  if (n == 0) return CA_OK;
  RvoDrawAtArgs q;
  std::memset(&q, 0, sizeof(q));
  q.seed = rd->seed; q.c = rd->collab_coeff; q.std = rd->noise_std;
  q.g = g; q.k = k; q.a = a; q.s = s; q.n = static_cast<long>(n);
  q.out_draw = out_noncoop_draw; q.out_noise = out_noise;
  const unsigned grid = static_cast<unsigned>((n + 255) / 256);
  return launch(rvo_draw_at_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), q);
}

int cagpu_ga3c_sample(const CaParams* p, const CaState* s, const CaAutoReset* ar, const CaPolicyDraw* draw, const CaMapSet* set,
                      const CaRvoDraw* rd, const CaGa3cSample* g, double* ext_actions, void* stream) {
  if (!p || !s || !g || !ext_actions || !g->logits || !g->logp || !s->flags || !s->step_num || !s->reset_count)
    return fail(CA_EINVAL, "cagpu_ga3c_sample: NULL pointer (p, s, g, ext_actions, logits, logp, flags, step_num, reset_count)%s");
  if (p->num_envs < 1 || p->num_agents < 1 || p->num_agents > big::NT_MAX || p->max_obs < 0)
    return fail(CA_EINVAL, "cagpu_ga3c_sample: bad sizes (num_agents outside 1..1024)%s");
  if (!g->greedy) {
    if (g->seed == 0) return fail(CA_EINVAL, "cagpu_ga3c_sample: CaGa3cSample.seed must not be 0%s");
    if ((ar && g->seed == ar->heading_seed) || (draw && g->seed == draw->seed) || (set && g->seed == set->map_seed) ||
        (rd && g->seed == rd->seed))
      return fail(CA_EINVAL, "cagpu_ga3c_sample: CaGa3cSample.seed equals CaAutoReset.heading_seed, CaPolicyDraw.seed, CaMapSet.map_seed "
                             "or CaRvoDraw.seed (two rules would read the same uniforms)%s");
  }
  if (!(g->temperature > 0.0f) || !(g->temperature < INFINITY))
    return fail(CA_EINVAL, "cagpu_ga3c_sample: CaGa3cSample.temperature must be > 0 and finite%s");
  if (reinterpret_cast<uintptr_t>(g->address) & 7u) return fail(CA_EINVAL, "cagpu_ga3c_sample: CaGa3cSample.address must be 8-byte aligned%s");
  if ((g->slot_obs && !g->obs) || (g->slot_value && !g->value))
    return fail(CA_EINVAL, "cagpu_ga3c_sample: slot_obs needs obs and slot_value needs value%s");
  sample::Args k;
  std::memset(&k, 0, sizeof(k));
  k.seed = g->greedy ? 0ull : g->seed;
  k.inv_T = 1.0f / g->temperature;
  k.greedy = g->greedy;
  k.mask = g->mask; k.agent_net = g->agent_net; k.net_index = g->net_index; k.address = g->address;
  k.logits = g->logits; k.flags = s->flags; k.step_num = s->step_num; k.reset_count = s->reset_count;
  k.env_id_offset = ar ? static_cast<long>(ar->env_id_offset) : 0;
  k.B = static_cast<long>(p->num_envs) * p->num_agents;
  k.N = p->num_agents; k.W = 6 + 7 * p->max_obs;
  k.ext = ext_actions; k.logp = g->logp; k.entropy = g->entropy; k.action = g->action;
  k.obs = g->obs; k.value = g->value;
  k.slot_obs = g->slot_obs; k.slot_value = g->slot_value; k.slot_live = g->slot_live; k.slot_address = g->slot_address;
  const unsigned grid = static_cast<unsigned>((k.B + sample::NT - 1) / sample::NT);
  return launch(sample::sample_kernel, dim3(grid), dim3(sample::NT), 0, static_cast<hipStream_t>(stream), k);
}

int cagpu_ga3c_sample_at(uint64_t seed, float temperature, int32_t num_agents, const int64_t* g, const int32_t* k, const int32_t* a,
                         const int32_t* s, const float* logits, int64_t n, int8_t* action, float* logp, float* entropy,
                         void* stream) {
  if (!g || !k || !a || !s || !logits || (!action && !logp && !entropy) || num_agents < 1 || num_agents > big::NT_MAX || n < 0)
    return fail(CA_EINVAL, "cagpu_ga3c_sample_at: NULL pointer, no output, num_agents outside 1..1024 or n < 0%s");
  if (seed == 0) return fail(CA_EINVAL, "cagpu_ga3c_sample_at: seed must not be 0%s");
  if (!(temperature > 0.0f) || !(temperature < INFINITY))
    return fail(CA_EINVAL, "cagpu_ga3c_sample_at: temperature must be > 0 and finite%s");
  if (n == 0) return CA_OK;
  sample::AtArgs q;
  std::memset(&q, 0, sizeof(q));
  q.seed = seed; q.inv_T = 1.0f / temperature;
  q.g = g; q.k = k; q.a = a; q.s = s; q.logits = logits; q.n = static_cast<long>(n);
  q.action = action; q.logp = logp; q.entropy = entropy;
  const unsigned grid = static_cast<unsigned>((n + sample::NT - 1) / sample::NT);
  return launch(sample::sample_at_kernel, dim3(grid), dim3(sample::NT), 0, static_cast<hipStream_t>(stream), q);
}

int cagpu_gae(int32_t n, int64_t EN, int32_t num_agents, const float* reward, const float* value, const float* last_value,
              const uint8_t* live, const uint8_t* done, const uint8_t* game_over, float gamma, float lambda, float* adv, float* ret,
              void* stream) {
  if (!reward || !value || !last_value || !live || !done || !game_over || !adv || !ret)
    return fail(CA_EINVAL, "cagpu_gae: NULL pointer%s");
  if (n < 1 || EN < 1 || num_agents < 1 || EN % num_agents != 0)
    return fail(CA_EINVAL, "cagpu_gae: n < 1, EN < 1 or EN not a multiple of num_agents%s");
  if (!(gamma >= 0.0f && gamma <= 1.0f) || !(lambda >= 0.0f && lambda <= 1.0f))
    return fail(CA_EINVAL, "cagpu_gae: gamma and lambda must lie in [0, 1]%s");
  sample::GaeArgs q;
  std::memset(&q, 0, sizeof(q));
  q.n = n; q.EN = static_cast<long>(EN); q.N = num_agents;
  q.reward = reward; q.value = value; q.last_value = last_value; q.live = live; q.done = done; q.game_over = game_over;
  q.gamma = gamma; q.gl = gamma * lambda;
  q.adv = adv; q.ret = ret;
  const unsigned grid = static_cast<unsigned>((EN + sample::NT - 1) / sample::NT);
  return launch(sample::gae_kernel, dim3(grid), dim3(sample::NT), 0, static_cast<hipStream_t>(stream), q);
}

int cagpu_map_draw(uint64_t seed, int32_t num_maps, const int64_t* env_ids, const int32_t* counts, int64_t n, int32_t* out,
                   void* stream) {
  if (!env_ids || !counts || !out || seed == 0 || num_maps < 1 || n < 0)
    return fail(CA_EINVAL, "cagpu_map_draw: NULL pointer, seed == 0, num_maps < 1 or n < 0%s");
  if (n == 0) return CA_OK;
  const unsigned grid = static_cast<unsigned>((n + 255) / 256);
  return launch(map_draw_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), seed, num_maps, env_ids, counts,
                static_cast<long>(n), out);
}

int cagpu_heading_draw(uint64_t heading_seed, int32_t num_agents, const int64_t* env_ids, const int32_t* counts, int64_t n,
                       double* out, void* stream) {
  if (!env_ids || !counts || !out || heading_seed == 0 || num_agents < 1 || num_agents > big::NT_MAX || n < 0)
    return fail(CA_EINVAL, "cagpu_heading_draw: NULL pointer, heading_seed == 0, num_agents outside 1..1024 or n < 0%s");
  if (n == 0) return CA_OK;
  const long total = static_cast<long>(n) * num_agents;
  const unsigned grid = static_cast<unsigned>((total + 255) / 256);
  return launch(heading_draw_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), heading_seed, num_agents,
                env_ids, counts, total, out);
}

int cagpu_policy_draw_at(const CaPolicyDraw* d, int32_t num_agents, const int64_t* env_ids, const int32_t* counts,
                         const uint8_t* present, int64_t n, uint32_t* out_bits, void* stream) {
  if (!d || !env_ids || !counts || !out_bits || num_agents < 1 || num_agents > big::NT_MAX || n < 0)
    return fail(CA_EINVAL, "cagpu_policy_draw_at: NULL pointer, num_agents outside 1..1024 or n < 0%s");
  const int rd = check_draw_pool(d, "cagpu_policy_draw_at");
  if (rd) return rd;
  if (n == 0) return CA_OK;
  DrawAtArgs k;
  std::memset(&k, 0, sizeof(k));
  k.cdf = d->cdf; k.bits = d->policy_bits; k.seed = d->seed; k.env_ids = env_ids; k.counts = counts; k.present = present;
  k.out = out_bits; k.n = static_cast<long>(n); k.N = num_agents; k.P = d->num_policies; k.ensure = d->ensure;
  const unsigned grid = static_cast<unsigned>(n < 65536 ? n : 65536);   // (one wave per pair; longer lists stride)
  return launch(policy_draw_at_kernel, dim3(grid), dim3(64), 0, static_cast<hipStream_t>(stream), k);
}

int cagpu_policy_draw(const CaParams* p, const CaState* s, const CaOut* o, const CaAutoReset* ar, const CaPolicyDraw* d,
                      const uint8_t* env_mask, void* stream) {
  if (!p || !s || !d) return fail(CA_EINVAL, "cagpu_policy_draw: NULL argument%s");
  const int rd = check_draw(d, ar, "cagpu_policy_draw");
  if (rd) return rd;
  if (p->num_envs < 1 || p->num_agents < 1 || p->num_agents > big::NT_MAX || p->max_obs < 0)
    return fail(CA_EINVAL, "cagpu_policy_draw: bad sizes%s");
  if (!s->flags || !s->reset_count) return fail(CA_EINVAL, "cagpu_policy_draw: NULL state pointer%s");
  if (o && !o->obs) return fail(CA_EINVAL, "cagpu_policy_draw: CaOut given with a NULL obs%s");
  DrawArgs k;
  std::memset(&k, 0, sizeof(k));
  k.flags = s->flags; k.reset_count = s->reset_count; k.obs = o ? o->obs : nullptr; k.mask = env_mask;
  k.cdf = d->cdf; k.bits = d->policy_bits; k.seed = d->seed;
  k.env_id_offset = ar->env_id_offset; k.total = static_cast<long>(p->num_envs) * p->num_agents;
  k.N = p->num_agents; k.W = 6 + 7 * p->max_obs; k.P = d->num_policies; k.ensure = d->ensure; k.ragged = p->ragged;
  const unsigned grid = static_cast<unsigned>((k.total + 255) / 256);
  return launch(policy_draw_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), k);
}

// The eleven fixed entry points: each is the CaStepEx its arguments spell, plus the record it insists on.
int cagpu_step(const CaParams* p, const CaState* s, const CaOut* o, const double* ext_actions, const CaAutoReset* ar,
               void* stream) {
  StepCall c;
  c.who = "cagpu_step";
  return step_impl(p, s, o, ext_actions, ar, c, stream);
}

int cagpu_step_map(const CaParams* p, const CaState* s, const CaOut* o, const double* ext_actions, const CaAutoReset* ar,
                   const CaMap* map, void* stream) {
  StepCall c;
  c.who = "cagpu_step_map"; c.map = map;
  return step_impl(p, s, o, ext_actions, ar, c, stream);
}

int cagpu_step_maps(const CaParams* p, const CaState* s, const CaOut* o, const double* ext_actions, const CaAutoReset* ar,
                    const CaMapSet* set, void* stream) {
  StepCall c;
  c.who = "cagpu_step_maps"; c.set = set; c.need = StepCall::NEED_SET;
  return step_impl(p, s, o, ext_actions, ar, c, stream);
}

int cagpu_step_traj(const CaParams* p, const CaState* s, const CaOut* o, const double* ext_actions, const CaAutoReset* ar,
                    const CaMap* map, const CaMapSet* set, const CaTraj* traj, void* stream) {
  StepCall c;
  c.who = "cagpu_step_traj"; c.map = map; c.set = set; c.traj = traj; c.need = StepCall::NEED_TRAJ;
  return step_impl(p, s, o, ext_actions, ar, c, stream);
}

int cagpu_rollout_traj(const CaParams* p, const CaState* s, const CaOut* o, const double* ext_actions, const CaAutoReset* ar,
                       int32_t n_steps, int32_t ring, int64_t snapshot_delta, const CaTraj* traj, void* stream) {
  StepCall c;
  c.who = "cagpu_rollout_traj"; c.n_steps = n_steps; c.ring = ring != 0; c.snapshot_delta = snapshot_delta;
  c.traj = traj; c.need = StepCall::NEED_TRAJ;
  return step_impl(p, s, o, ext_actions, ar, c, stream);
}

int cagpu_step_final(const CaParams* p, const CaState* s, const CaOut* o, const double* ext_actions, const CaAutoReset* ar,
                     const CaMap* map, const CaMapSet* set, const CaTraj* traj, const CaFinal* fin, void* stream) {
  StepCall c;
  c.who = "cagpu_step_final"; c.map = map; c.set = set; c.traj = traj; c.fin = fin; c.need = StepCall::NEED_FIN;
  return step_impl(p, s, o, ext_actions, ar, c, stream);
}

int cagpu_rollout_final(const CaParams* p, const CaState* s, const CaOut* o, const double* ext_actions, const CaAutoReset* ar,
                        int32_t n_steps, int32_t ring, int64_t snapshot_delta, const CaTraj* traj, const CaFinal* fin,
                        void* stream) {
  StepCall c;
  c.who = "cagpu_rollout_final"; c.n_steps = n_steps; c.ring = ring != 0; c.snapshot_delta = snapshot_delta;
  c.traj = traj; c.fin = fin; c.need = StepCall::NEED_FIN;
  return step_impl(p, s, o, ext_actions, ar, c, stream);
}

int cagpu_step_log(const CaParams* p, const CaState* s, const CaOut* o, const double* ext_actions, const CaAutoReset* ar,
                   const CaMap* map, const CaMapSet* set, const CaTraj* traj, const CaFinal* fin, const CaEpLog* log,
                   void* stream) {
  StepCall c;
  c.who = "cagpu_step_log"; c.map = map; c.set = set; c.traj = traj; c.fin = fin; c.log = log; c.need = StepCall::NEED_LOG;
  return step_impl(p, s, o, ext_actions, ar, c, stream);
}

int cagpu_rollout_log(const CaParams* p, const CaState* s, const CaOut* o, const double* ext_actions, const CaAutoReset* ar,
                      int32_t n_steps, int32_t ring, int64_t snapshot_delta, const CaTraj* traj, const CaFinal* fin,
                      const CaEpLog* log, void* stream) {
  StepCall c;
  c.who = "cagpu_rollout_log"; c.n_steps = n_steps; c.ring = ring != 0; c.snapshot_delta = snapshot_delta;
  c.traj = traj; c.fin = fin; c.log = log; c.need = StepCall::NEED_LOG;
  return step_impl(p, s, o, ext_actions, ar, c, stream);
}

// idx_out: the slot march (cagpu_laserscan_slots) -- scan_kernel<true> writes the new index rows there and no history
static int laserscan_impl(const CaParams* p, const CaState* s, const CaMap* map, const CaScan* scan, void* stream,
                          const CaMapSet* set = nullptr, uint8_t* idx_out = nullptr) {
  if (!p || !s || !map || !scan) return fail(CA_EINVAL, "cagpu_laserscan: NULL argument%s");
  if (p->num_envs < 1 || p->num_agents < 1 || p->num_agents > 256) return fail(CA_EINVAL, "cagpu_laserscan: bad sizes%s");
  if (map->rows < 1 || map->cols < 1 || !(map->cell > 0.0)) return fail(CA_EINVAL, "cagpu_laserscan: bad CaMap%s");
  if ((!idx_out && (!scan->hist || !scan->out)) || scan->num_beams < 2 || scan->num_to_store < 1 || scan->num_ranges < 1 ||
      scan->num_ranges > 255)
    return fail(CA_EINVAL, "cagpu_laserscan: bad CaScan%s");
  if (!s->pos_x || !s->pos_y || !s->heading || !s->radius || !s->step_num) return fail(CA_EINVAL, "cagpu_laserscan: NULL state pointer%s");
  if (!(scan->range_res / map->cell + 0.2 < SCAN_PAD - 1))
    return fail(CA_EUNSUPPORTED, "cagpu_laserscan: range_res above 6 cells is not supported (LDS bitmap border)%s");
  // (beams are clipped to the grid box + 1 cm, and the march starts up to a sample before that: scan_kernel's `slack`)
  if (!((scan->range_res + 0.01) / map->cell + 0.2 < SCAN_PAD))
    return fail(CA_EUNSUPPORTED, "cagpu_laserscan: range_res + 1 cm above 7.8 cells is not supported (LDS bitmap border)%s");
  ScanArgs k;
  std::memset(&k, 0, sizeof(k));
  k.p = *p; k.s = *s; k.m = *map; k.sc = *scan;
  if (set) { k.env_map = set->env_map; k.num_maps = set->num_maps; }
  if (idx_out) { k.sc.hist = idx_out; k.sc.out = nullptr; }  // (scan_kernel<true>: the index rows go where the history would)
  const int N = p->num_agents;
  const size_t total = align16(scan_grid_words(map->rows, map->cols) * 4) + static_cast<size_t>(N) * (4 * 8 + 2 * 8 + 3 * 4 + 2 * 8 + 2 * 8 + 3 * 4 + 4 * 4) +
                       static_cast<size_t>(scan->num_beams) * 16 + 256 * 4 + 32 + static_cast<size_t>(HIST_AG) * SCAN_NT;
  if (total > 160 * 1024) return fail(CA_EUNSUPPORTED, "cagpu_laserscan: map too large for the LDS bitmap%s");
  return launch_lds(idx_out ? kernel_of<&scan_kernel<true>>() : kernel_of<&scan_kernel<false>>(),
                    dim3(static_cast<unsigned>(p->num_envs)), dim3(SCAN_NT), total, static_cast<hipStream_t>(stream), k);
}

int cagpu_laserscan(const CaParams* p, const CaState* s, const CaMap* map, const CaScan* scan, void* stream) {
  return laserscan_impl(p, s, map, scan, stream);
}

int cagpu_laserscan_maps(const CaParams* p, const CaState* s, const CaMapSet* set, const CaScan* scan, void* stream) {
  const int rc = check_map_set(set, "cagpu_laserscan_maps");
  if (rc) return rc;
  return laserscan_impl(p, s, &set->map, scan, stream, set);
}

static int occupancy_impl(const CaParams* p, const CaState* s, const CaMap* map, const CaOccGrid* g, void* stream,
                          const CaMapSet* set = nullptr) {
  if (!p || !s || !map || !g) return fail(CA_EINVAL, "cagpu_occupancy_grid: NULL argument%s");
  if (p->num_envs < 1 || p->num_agents < 1 || p->num_agents > big::NT_MAX) return fail(CA_EINVAL, "cagpu_occupancy_grid: bad sizes%s");
  if (map->rows < 1 || map->cols < 1 || !(map->cell > 0.0)) return fail(CA_EINVAL, "cagpu_occupancy_grid: bad CaMap%s");
  if (!g->cells && !g->bits) return fail(CA_EINVAL, "cagpu_occupancy_grid: CaOccGrid.cells and .bits are both NULL%s");
  if (g->height < 1 || g->height > 256 || g->width < 1 || g->width > 256)
    return fail(CA_EINVAL, "cagpu_occupancy_grid: height and width must be in [1, 256]%s");
  if ((reinterpret_cast<uintptr_t>(g->cells) | reinterpret_cast<uintptr_t>(g->bits)) & 15)
    return fail(CA_EINVAL, "cagpu_occupancy_grid: output pointers must be 16-byte aligned%s");
  if (!s->pos_x || !s->pos_y || !s->radius) return fail(CA_EINVAL, "cagpu_occupancy_grid: NULL state pointer%s");
  const size_t bitmap = static_cast<size_t>(map->rows) * ((static_cast<size_t>(map->cols) + 31) / 32) * 4;
  if (bitmap > 128 * 1024) return fail(CA_EUNSUPPORTED, "cagpu_occupancy_grid: map too large for the LDS bitmap%s");
  OccArgs k;
  std::memset(&k, 0, sizeof(k));
  k.p = *p; k.s = *s; k.m = *map; k.g = *g;
  if (set) { k.env_map = set->env_map; k.num_maps = set->num_maps; }
  const size_t total = occ_lds_bytes(map->rows, map->cols, p->num_agents);
  return launch_lds(kernel_of<&occ_kernel>(), dim3(static_cast<unsigned>(p->num_envs)), dim3(OCC_NT), total,
                    static_cast<hipStream_t>(stream), k);
}

int cagpu_occupancy_grid(const CaParams* p, const CaState* s, const CaMap* map, const CaOccGrid* g, void* stream) {
  return occupancy_impl(p, s, map, g, stream);
}

int cagpu_occupancy_grid_maps(const CaParams* p, const CaState* s, const CaMapSet* set, const CaOccGrid* g, void* stream) {
  const int rc = check_map_set(set, "cagpu_occupancy_grid_maps");
  if (rc) return rc;
  return occupancy_impl(p, s, &set->map, g, stream, set);
}

static int render_impl(const CaParams* p, const CaState* s, const CaMap* map, const CaRender* r, void* stream,
                       const CaMapSet* set = nullptr) {
  if (!p || !s || !r) return fail(CA_EINVAL, "cagpu_render: NULL argument%s");
  if (p->num_envs < 1 || p->num_agents < 1 || p->num_agents > big::NT_MAX) return fail(CA_EINVAL, "cagpu_render: bad sizes%s");
  if (!s->pos_x || !s->pos_y || !s->goal_x || !s->goal_y || !s->radius || !s->flags)
    return fail(CA_EINVAL, "cagpu_render: NULL state pointer%s");
  if (!r->out || (reinterpret_cast<uintptr_t>(r->out) & 15)) return fail(CA_EINVAL, "cagpu_render: output NULL or not 16-byte aligned%s");
  if (r->num_frames < 1 || r->height < 16 || r->height > 1024 || r->width < 16 || r->width > 1024)
    return fail(CA_EINVAL, "cagpu_render: num_frames < 1, or height / width outside [16, 1024]%s");
  if (!(r->s16 > 0.0) || !(r->s16 <= 1e9) || !(r->xmin - r->xmin == 0.0) || !(r->ymax - r->ymax == 0.0))
    return fail(CA_EINVAL, "cagpu_render: bad window (xmin, ymax must be finite, 0 < s16 <= 1e9)%s");
  if (!r->frame_env || !r->first || !r->last) return fail(CA_EINVAL, "cagpu_render: NULL frame_env / first / last%s");
  if (r->hist_steps < 0 || (r->hist_steps > 0 && (!r->hist || r->hist_cols < 1 || r->stride_s < 0 || r->stride_t < 0)))
    return fail(CA_EINVAL, "cagpu_render: bad history block%s");
  if (r->hist && (reinterpret_cast<uintptr_t>(r->hist) & 15)) return fail(CA_EINVAL, "cagpu_render: history not 16-byte aligned%s");
  const bool has_map = map && map->static_bits;
  if (has_map && (map->rows < 1 || map->cols < 1 || !(map->cell > 0.0))) return fail(CA_EINVAL, "cagpu_render: bad CaMap%s");
  const int T = r->hist ? r->hist_steps : 0;
  if (render_cap(p->num_agents, T) > 0x7FFFFFFFu) return fail(CA_EUNSUPPORTED, "cagpu_render: too many history rows per frame%s");
  if (!r->work || (reinterpret_cast<uintptr_t>(r->work) & 15) || r->work_bytes < render_work_bytes(r->num_frames, p->num_agents, T))
    return fail(CA_EINVAL, "cagpu_render: workspace NULL, not 16-byte aligned or smaller than cagpu_render_work_bytes()%s");
  RenderArgs k;
  std::memset(&k, 0, sizeof(k));
  k.p = *p; k.s = *s; k.r = *r;
  if (has_map) k.m = *map;
  if (!r->hist) k.r.hist_steps = 0;
  if (set) { k.env_map = set->env_map; k.num_maps = set->num_maps; }
  k.cap = static_cast<int32_t>(render_cap(p->num_agents, T));
  const int u = r->width > r->height ? r->width : r->height;
  k.g16 = (291 * u) / 1000 < 32 ? 32 : (291 * u) / 1000;
  k.d16 = (108 * u) / 1000 < 16 ? 16 : (108 * u) / 1000;
  k.tiles_x = (r->width + RD_TW - 1) / RD_TW;
  k.tiles_y = (r->height + RD_TH - 1) / RD_TH;
  const long blocks = static_cast<long>(k.tiles_x) * k.tiles_y * r->num_frames;
  if (blocks > 0x7FFFFFFFL) return fail(CA_EUNSUPPORTED, "cagpu_render: more than 2^31 - 1 (frame, tile) workgroups%s");
  const int N = p->num_agents;
  const size_t lds = static_cast<size_t>(N) * (8 + 7 * 4) + 8 + 16;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (const int rc = launch(render_prep_kernel, dim3(static_cast<unsigned>(r->num_frames)), dim3(RD_NT), lds, st, k)) return rc;
  return launch(render_raster_kernel, dim3(static_cast<unsigned>(blocks)), dim3(RD_NT), 0, st, k);
}

uint64_t cagpu_render_work_bytes(int32_t num_frames, int32_t num_agents, int32_t hist_steps) {
  if (num_frames < 1 || num_agents < 1 || hist_steps < 0) return 0;
  return render_work_bytes(num_frames, num_agents, hist_steps);
}

int cagpu_render(const CaParams* p, const CaState* s, const CaMap* map, const CaRender* r, void* stream) {
  return render_impl(p, s, map, r, stream);
}

int cagpu_render_maps(const CaParams* p, const CaState* s, const CaMapSet* set, const CaRender* r, void* stream) {
  const int rc = check_map_set(set, "cagpu_render_maps");
  if (rc) return rc;
  return render_impl(p, s, &set->map, r, stream, set);
}

static int ga3c_check_net(const CaNet* net) {
  const void* w[] = {net->lstm_kernel, net->lstm_bias, net->layer1_kernel, net->layer1_bias, net->layer2_kernel,
                     net->layer2_bias, net->fc1_kernel, net->fc1_bias, net->logits_kernel, net->logits_bias,
                     net->input_mean, net->input_std};
  for (const void* q : w)
    if (!q || (reinterpret_cast<uintptr_t>(q) & 15)) return fail(CA_EINVAL, "cagpu_ga3c: NULL or not 16-byte aligned weight pointer%s");
  if (!net->packed || (reinterpret_cast<uintptr_t>(net->packed) & 15))
    return fail(CA_EINVAL, "cagpu_ga3c: CaNet.packed is NULL or not 16-byte aligned (fill it once per checkpoint with cagpu_ga3c_pack)%s");
  return CA_OK;
}
// The launch of ga3c_kernel<true> (the query rows / the value head): its own instantiation, its own LDS limit.
static int ga3c_launch_ext(ga3c::Args& k, const ga3c::Ext& ex, void* stream) {
  constexpr size_t lds = ga3c::LDS_BYTES;
  k.slots = 2 * device_cus();
  k.force_tile = 0;
  const unsigned grid = static_cast<unsigned>((k.B + 31) / 32);  // (B < 2^31)
  std::snprintf(g_last_kernel, sizeof(g_last_kernel), "ga3c_kernel<true> %s grid=%u lds=%zu rows=%ld width=%d%s%s%s",
                ex.query ? "query" : "sim", grid, lds, k.B, k.W - 1, k.logits ? " logits" : "",
                ex.value ? " value" : "", ex.action ? " action" : "");
  return launch_lds(kernel_of<&ga3c::ga3c_kernel<true>>(), dim3(grid), dim3(ga3c::NT), lds, static_cast<hipStream_t>(stream), k, ex);
}

static int ga3c_impl(const CaParams* p, const CaState* s, const float* obs, const CaNet* net, double* ext_actions, float* logits,
                     const CaNetValue* val, void* stream) {
  if (!p || !s || !net || !ext_actions) return fail(CA_EINVAL, "cagpu_ga3c: NULL argument%s");
  if (!obs) {  // fused sensing: the kernel computes the observation rows it needs from the state
    if (p->num_agents > 32 || p->sort_mode == CA_SORT_TIME_TO_IMPACT)
      return fail(CA_EUNSUPPORTED, "cagpu_ga3c: fused sensing (obs == NULL) needs num_agents <= 32 and closest_first / closest_last sorting%s");
    if (p->obs_clip < 0 || p->obs_clip > p->max_obs) return fail(CA_EINVAL, "cagpu_ga3c: obs_clip must be in [0, max_obs]%s");
    const void* q[] = {s->pos_x, s->pos_y, s->vel_x, s->vel_y, s->heading, s->goal_x, s->goal_y, s->radius, s->pref_speed};
    for (const void* x : q)
      if (!x) return fail(CA_EINVAL, "cagpu_ga3c: fused sensing needs the state arrays%s");
  }
  if (p->num_envs < 1 || p->num_agents < 1 || p->max_obs < 0) return fail(CA_EINVAL, "cagpu_ga3c: bad sizes%s");
  if (!s->flags) return fail(CA_EINVAL, "cagpu_ga3c: NULL state pointer%s");
  if (const int rc = ga3c_check_net(net)) return rc;
  ga3c::Args k;
  std::memset(&k, 0, sizeof(k));
  k.obs = obs; k.flags = s->flags;
  k.pos_x = s->pos_x; k.pos_y = s->pos_y; k.vel_x = s->vel_x; k.vel_y = s->vel_y; k.heading = s->heading;
  k.goal_x = s->goal_x; k.goal_y = s->goal_y; k.radius = s->radius; k.pref_speed = s->pref_speed;
  k.N = p->num_agents; k.K = p->max_obs; k.obs_clip = p->obs_clip; k.sort_mode = p->sort_mode; k.ragged = p->ragged;
  k.sensing_horizon = p->sensing_horizon;
  k.B = static_cast<long>(p->num_envs) * p->num_agents;
  k.W = 6 + 7 * p->max_obs;
  k.net = *net; k.ext = ext_actions; k.logits = logits;
  k.rows = net->rows_scratch;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (k.rows) {
    if (k.B >= (1L << 31)) return fail(CA_EUNSUPPORTED, "cagpu_ga3c: more than 2^31 agents with rows_scratch%s");
    // the packing's two counters are tagged with this call's epoch (compact_kernel): nothing to clear, whatever an earlier
    // launch or the caller's allocation left in the scratch; rows_scratch must hold num_envs * num_agents + 6 words
    const uint32_t epoch = next_pack_epoch();
    const int rc = launch(ga3c::compact_kernel, dim3(static_cast<unsigned>((k.B + 4 * ga3c::CP_NT - 1) / (4 * ga3c::CP_NT))),
                          dim3(ga3c::CP_NT), 0, st, s->flags, k.B, net->rows_scratch, net->agent_net, net->net_index, epoch);
    if (rc) return rc;
  }
  static_assert(ga3c::LDS_BYTES <= 80 * 1024, "two workgroups per CU");
  if (val) {  // the value head rides on the other instantiation; the default launch below is untouched
    ga3c::Ext ex;
    std::memset(&ex, 0, sizeof(ex));
    ex.value_kernel = val->value_kernel; ex.value_bias = val->value_bias; ex.value = val->value;
    return ga3c_launch_ext(k, ex, stream);
  }
  k.slots = 2 * device_cus();
  k.force_tile = 0;
  // the tile height (64 / 48 / 32 rows) is chosen on the device from the number of live rows: the grid covers the worst
  // case (32-row tiles); workgroups beyond the last tile leave at once
  const unsigned grid = static_cast<unsigned>((k.B + 31) / 32);
  return launch_lds(kernel_of<&ga3c::ga3c_kernel<false>>(), dim3(grid), dim3(ga3c::NT), ga3c::LDS_BYTES, st, k, ga3c::NoExt{});
}

int cagpu_ga3c(const CaParams* p, const CaState* s, const float* obs, const CaNet* net, double* ext_actions, float* logits,
               void* stream) {
  return ga3c_impl(p, s, obs, net, ext_actions, logits, nullptr, stream);
}

int cagpu_ga3c_value(const CaParams* p, const CaState* s, const float* obs, const CaNet* net, double* ext_actions, float* logits,
                     const CaNetValue* v, void* stream) {
  if (v && (!v->value || !v->value_kernel || !v->value_bias))
    return fail(CA_EINVAL, "cagpu_ga3c_value: CaNetValue needs value, value_kernel and value_bias%s");
  if (v && p && static_cast<long>(p->num_envs) * p->num_agents >= (1L << 31))  // (the value launch indexes rows as int32)
    return fail(CA_EUNSUPPORTED, "cagpu_ga3c_value: more than 2^31 agents%s");
  return ga3c_impl(p, s, obs, net, ext_actions, logits, v, stream);
}

int cagpu_ga3c_query(const CaNet* net, const CaNetQuery* q, void* stream) {
  if (!net || !q || !q->x) return fail(CA_EINVAL, "cagpu_ga3c_query: NULL argument%s");
  if (q->rows < 0 || q->width < 1) return fail(CA_EINVAL, "cagpu_ga3c_query: rows must be >= 0 and width >= 1%s");
  if (q->value && (!q->value_kernel || !q->value_bias))
    return fail(CA_EINVAL, "cagpu_ga3c_query: value needs value_kernel and value_bias (logits_v)%s");
  if (!q->logits && !q->value && !q->action) return fail(CA_EINVAL, "cagpu_ga3c_query: no output requested%s");
  if (const int rc = ga3c_check_net(net)) return rc;
  if (q->rows == 0) return CA_OK;
  if (q->rows >= (1LL << 31)) return fail(CA_EUNSUPPORTED, "cagpu_ga3c_query: 2^31 rows or more in one call%s");
  ga3c::Args k;
  std::memset(&k, 0, sizeof(k));
  k.obs = q->x;
  k.B = static_cast<long>(q->rows);
  k.W = q->width + 1;  // (the kernel's W counts the is_learning column a query row does not have)
  k.net = *net;
  k.net.agent_net = nullptr;
  k.logits = q->logits;
  ga3c::Ext ex;
  std::memset(&ex, 0, sizeof(ex));
  ex.query = 1;
  if (q->value) { ex.value_kernel = q->value_kernel; ex.value_bias = q->value_bias; ex.value = q->value; }
  ex.action = q->action;
  return ga3c_launch_ext(k, ex, stream);
}

// ---- the weight gradients of the GA3C-CADRL network (csrc/cagpu_ga3c_grad.inc)
uint64_t cagpu_ga3c_grad_floats(void) { return static_cast<uint64_t>(ga3c_grad::G_TOTAL); }

uint64_t cagpu_ga3c_grad_work_bytes(int64_t rows) {
  if (rows <= 0 || rows >= (1LL << 31)) return 0;  // (rows == 0: the call launches nothing and needs no workspace)
  return static_cast<uint64_t>(ga3c_grad::layout_of(static_cast<long>(rows)).total) * sizeof(float);
}

int cagpu_ga3c_grad(const CaNet* net, const CaNetGrad* q, void* stream) {
  namespace gg = ga3c_grad;
  if (!net || !q || !q->grad) return fail(CA_EINVAL, "cagpu_ga3c_grad: NULL argument (net, g or grad)%s");
  if (q->rows != 0 && (!q->x || !q->work)) return fail(CA_EINVAL, "cagpu_ga3c_grad: NULL x or work%s");
  if (q->rows < 0 || q->width < 1) return fail(CA_EINVAL, "cagpu_ga3c_grad: rows must be >= 0 and width >= 1%s");
  if (!q->dlogits && !q->dvalue) return fail(CA_EINVAL, "cagpu_ga3c_grad: dlogits and dvalue are both NULL%s");
  if (q->dvalue && (!q->value_kernel || !q->value_bias))
    return fail(CA_EINVAL, "cagpu_ga3c_grad: dvalue needs value_kernel and value_bias (logits_v)%s");
  const void* w[] = {net->lstm_kernel, net->lstm_bias, net->layer1_kernel, net->layer1_bias, net->layer2_kernel, net->layer2_bias,
                     net->fc1_kernel, net->fc1_bias, net->logits_kernel, net->logits_bias, net->input_mean, net->input_std};
  for (const void* p : w)
    if (!p) return fail(CA_EINVAL, "cagpu_ga3c_grad: NULL weight pointer%s");
  if (q->rows >= (1LL << 31)) return fail(CA_EUNSUPPORTED, "cagpu_ga3c_grad: 2^31 rows or more in one call%s");
  if (q->work_bytes < cagpu_ga3c_grad_work_bytes(q->rows))
    return fail(CA_EINVAL, "cagpu_ga3c_grad: work_bytes is below cagpu_ga3c_grad_work_bytes(rows)%s");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (q->rows == 0) {
    if (!q->accumulate && hipMemsetAsync(q->grad, 0, gg::G_TOTAL * sizeof(float), st) != hipSuccess)
      return fail(CA_ELAUNCH, "cagpu_ga3c_grad: hipMemsetAsync failed%s");
    return CA_OK;
  }
  gg::Args k;
  std::memset(&k, 0, sizeof(k));
  k.x = q->x; k.rows = static_cast<long>(q->rows); k.width = q->width; k.live = q->live;
  k.dlogits = q->dlogits; k.dvalue = q->dvalue;
  k.net = *net;
  k.value_kernel = q->value_kernel;
  k.work = static_cast<float*>(q->work);
  k.l = gg::layout_of(k.rows);
  const gg::Layout& l = k.l;
  if (const int rc = launch(gg::prep_kernel, dim3(static_cast<unsigned>((gg::WT_TOTAL + 255) / 256)), dim3(256), 0, st, k.net,
                            k.value_kernel, k.work))
    return rc;
  const unsigned grid = static_cast<unsigned>((k.rows + gg::T - 1) / gg::T);
  std::snprintf(g_last_kernel, sizeof(g_last_kernel), "ga3c_grad_kernel grid=%u lds=%zu rows=%ld width=%d slices=%d%s%s%s%s", grid,
                gg::LDS_BYTES, k.rows, k.width, l.slices, k.dlogits ? " logits" : "", k.dvalue ? " value" : "",
                k.live ? " live" : "", q->accumulate ? " accumulate" : "");
  if (const int rc = launch_lds(kernel_of<&gg::ga3c_grad_kernel>(), dim3(grid), dim3(gg::NT), gg::LDS_BYTES, st, k)) return rc;
  gg::WArgs wa;
  std::memset(&wa, 0, sizeof(wa));
  const long R = k.rows;
  //                   A      dZ     M        lda  K   ldz  N    out           ldo  bias
  wa.job[0] = gg::WJob{l.xo,  l.dzl, R * 19,  7,   7,  256, 256, gg::G_LSTM_K, 256, gg::G_LSTM_B};
  wa.job[1] = gg::WJob{l.hp,  l.dzl, R * 19,  64,  64, 256, 256, gg::G_LSTM_K + 7 * 256, 256, -1};
  wa.job[2] = gg::WJob{l.a0,  l.dz1, R,       68,  68, 256, 256, gg::G_L1_K,   256, gg::G_L1_B};
  wa.job[3] = gg::WJob{l.a1,  l.dz2, R,       256, 256, 256, 256, gg::G_L2_K,  256, gg::G_L2_B};
  wa.job[4] = gg::WJob{l.a2,  l.dz3, R,       256, 256, 256, 256, gg::G_FC_K,  256, gg::G_FC_B};
  wa.job[5] = gg::WJob{l.a3,  l.dzh, R,       256, 256, gg::NHEAD, 11, gg::G_P_K, 11, gg::G_P_B};
  wa.job[6] = gg::WJob{l.a3,  l.dzh + 11, R,  256, 256, gg::NHEAD, 1, gg::G_V_K, 1, gg::G_V_B};
  wa.work = k.work; wa.part = l.part; wa.slices = l.slices;
  if (const int rc = launch(gg::wgrad_kernel, dim3(l.slices, 256 / gg::KB, gg::NJOBS), dim3(gg::NT), 0, st, wa)) return rc;
  return launch(gg::reduce_kernel, dim3((gg::G_TOTAL + 255) / 256), dim3(256), 0, st,
                static_cast<const float*>(k.work + l.part), l.slices, q->grad, q->accumulate ? 1 : 0);
}

// the generator's argument block from the entry points' arguments; `plain` / `ragged` name the caller in the messages
static int gen_fail(const char* who, const char* text) {
  std::snprintf(g_err, sizeof(g_err), "%s: %s", who, text);
  return CA_EINVAL;
}

static int generate_args(gen::Args& a, const char* plain, const char* ragged, int32_t num_agents, int32_t n_min, int32_t n_max,
                         const double* side_ranges, int32_t n_ranges, double side_lo, double side_hi, double speed_lo,
                         double speed_hi, double radius_lo, double radius_hi, uint64_t seed, double* cases, int32_t* counts,
                         int32_t* status) {
  if (!cases) return gen_fail(plain, "NULL cases");
  if (!(side_lo > 0.0) || !(side_hi >= side_lo) || !(speed_lo > 0.0) || !(speed_hi >= speed_lo) || !(radius_lo > 0.0) ||
      !(radius_hi >= radius_lo))
    return gen_fail(plain, "bounds must be positive and ordered");
  std::memset(&a, 0, sizeof(a));
  a.cases = cases; a.status = status; a.N = num_agents;
  a.side_lo = side_lo; a.side_hi = side_hi; a.speed_lo = speed_lo; a.speed_hi = speed_hi;
  a.radius_lo = radius_lo; a.radius_hi = radius_hi; a.seed = seed;
  a.max_attempts = 20000;  // the reference loops until a sample is accepted (its square / circle grows 1 % per retry)
  a.counts = counts;
  if (n_max > 0) {
    if (n_min < 1 || n_min > n_max || n_max > num_agents) return gen_fail(ragged, "need 1 <= n_min <= n_max <= max_agents");
    a.n_min = n_min; a.n_max = n_max;
  }
  if (n_ranges > 0) {
    if (n_ranges > 8 || !side_ranges) return gen_fail(ragged, "at most 8 side ranges");
    for (int r = 0; r < n_ranges; ++r) {
      for (int k = 0; k < 4; ++k) a.ranges[r][k] = side_ranges[r * 4 + k];
      if (!(a.ranges[r][2] > 0.0) || !(a.ranges[r][3] >= a.ranges[r][2]))
        return gen_fail(ragged, "side ranges must be positive and ordered");
    }
    a.n_ranges = n_ranges;
    // the reference asserts that some entry holds the drawn count (test_cases.py:241)
    for (int n = (n_max > 0 ? n_min : num_agents); n <= (n_max > 0 ? n_max : num_agents); ++n) {
      bool held = false;
      for (int r = 0; r < n_ranges; ++r) held = held || (a.ranges[r][0] <= n && n < a.ranges[r][1]);
      if (!held) return gen_fail(ragged, "an agent count in [n_min, n_max] has no side range");
    }
  }
  return CA_OK;
}

static int generate_impl(int64_t num_cases, int32_t num_agents, int32_t n_min, int32_t n_max, const double* side_ranges,
                         int32_t n_ranges, double side_lo, double side_hi, double speed_lo, double speed_hi, double radius_lo,
                         double radius_hi, uint64_t seed, double* cases, int32_t* counts, int32_t* status, void* stream) {
  if (num_cases < 1 || num_agents < 1 || num_agents > 4096) return fail(CA_EINVAL, "cagpu_generate_cases: bad sizes%s");
  gen::Args a;
  const int rc = generate_args(a, "cagpu_generate_cases", "cagpu_generate_cases_ragged", num_agents, n_min, n_max, side_ranges,
                               n_ranges, side_lo, side_hi, speed_lo, speed_hi, radius_lo, radius_hi, seed, cases, counts, status);
  if (rc != CA_OK) return rc;
  a.C = num_cases;
  return launch(gen::generate_kernel, dim3(static_cast<unsigned>((num_cases + 63) / 64)), dim3(64), 0,
                static_cast<hipStream_t>(stream), a);
}

// the wave-per-case launch over a list (cagpu_generate_cases_at, cagpu_stream_refill): grid and block depend on M only
static int launch_generate_at(const gen::Args& a, const int64_t* case_index, const int64_t* out_row, const int32_t* count,
                              int64_t M, void* stream) {
  gen::AtArgs q;
  q.a = a;
  q.case_index = reinterpret_cast<const long long*>(case_index);
  q.out_row = reinterpret_cast<const long long*>(out_row);
  q.count = count; q.M = static_cast<long>(M);
  const int64_t cap = 16L * device_cus();
  const unsigned grid = static_cast<unsigned>(M < cap ? M : cap);
  const size_t lds = static_cast<size_t>(a.N) * 6 * sizeof(double);
  return launch(gen::generate_at_kernel, dim3(grid), dim3(64), lds, static_cast<hipStream_t>(stream), q);
}

// side_ranges of the _at / stream form: n_ranges == 0 means HOST [2] = side lo, hi (the plain form of cagpu_generate_cases)
static int generate_at_args(gen::Args& a, const char* who, int32_t max_agents, int32_t n_min, int32_t n_max,
                            const double* side_ranges, int32_t n_ranges, double speed_lo, double speed_hi, double radius_lo,
                            double radius_hi, uint64_t seed, double* cases, int32_t* counts, int32_t* status) {
  if (max_agents < 1 || max_agents > 1024) return gen_fail(who, "max_agents must be in 1..1024");
  if (n_ranges < 0 || !side_ranges) return gen_fail(who, "side_ranges is NULL or n_ranges < 0");
  if (n_max < 0) return gen_fail(who, "need 1 <= n_min <= n_max <= max_agents");
  const bool plain = n_ranges == 0;
  return generate_args(a, who, who, max_agents, n_min, n_max, plain ? nullptr : side_ranges, n_ranges,
                       plain ? side_ranges[0] : 1.0, plain ? side_ranges[1] : 1.0, speed_lo, speed_hi, radius_lo, radius_hi, seed,
                       cases, counts, status);
}

int cagpu_generate_cases_at(const int64_t* case_index, const int64_t* out_row, const int32_t* count, int64_t M,
                            int32_t max_agents, int32_t n_min, int32_t n_max, const double* side_ranges, int32_t n_ranges,
                            double speed_lo, double speed_hi, double radius_lo, double radius_hi, uint64_t seed, double* cases,
                            int32_t* counts, int32_t* status, void* stream) {
  const char* who = "cagpu_generate_cases_at";
  if (M < 1 || M > 0x7FFFFFFFL) return gen_fail(who, "the list needs 1 .. 2^31 - 1 entries");
  if (!case_index) return gen_fail(who, "NULL case_index");
  gen::Args a;
  const int rc = generate_at_args(a, who, max_agents, n_min, n_max, side_ranges, n_ranges, speed_lo, speed_hi, radius_lo,
                                  radius_hi, seed, cases, counts, status);
  if (rc != CA_OK) return rc;
  return launch_generate_at(a, case_index, out_row, count, M, stream);
}

int cagpu_stream_refill(const CaParams* p, const CaState* s, const CaAutoReset* ar, const CaCaseStream* cs, void* stream) {
  const char* who = "cagpu_stream_refill";
  if (!p || !s || !ar || !cs) return gen_fail(who, "NULL argument");
  if (p->num_envs < 1 || p->num_agents < 1) return gen_fail(who, "bad sizes");
  if (!s->reset_count) return gen_fail(who, "NULL state pointer (reset_count)");
  if (cs->window < 1) return gen_fail(who, "window must be >= 1");
  const int64_t rows = static_cast<int64_t>(p->num_envs) * cs->window;
  if (rows > 0x7FFFFFFFL) return gen_fail(who, "num_envs * window does not fit CaAutoReset.n_cases");
  if (!cs->table || !cs->held || !cs->seen || !cs->work_index || !cs->work_row || !cs->work_count)
    return gen_fail(who, "NULL pointer in CaCaseStream (table, held, seen, work_index, work_row, work_count)");
  if (ar->table != cs->table || ar->n_cases != rows || ar->case_stride != p->num_envs)
    return gen_fail(who, "the CaAutoReset must name the window: table = CaCaseStream.table, n_cases = num_envs * window, "
                         "case_stride = num_envs");
  if (ar->reset_obs || ar->reset_plan)
    return gen_fail(who, "reset_obs / reset_plan of a stream's CaAutoReset must be NULL (the rows change under them)");
  if (ar->env_id_offset < 0 || ar->env_id_offset + p->num_envs > (1LL << 32))
    return gen_fail(who, "global env ids (env_id_offset + e) must be < 2^32");
  gen::Args a;
  const int rc = generate_at_args(a, who, p->num_agents, cs->n_min, cs->n_max, cs->side_ranges, cs->n_ranges, cs->speed_lo,
                                  cs->speed_hi, cs->radius_lo, cs->radius_hi, cs->seed, cs->table, cs->counts, cs->status);
  if (rc != CA_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(cs->work_count, 0, sizeof(int32_t), st);
  if (e != hipSuccess) return fail(CA_ELAUNCH, "cagpu_stream_refill: %s", hipGetErrorString(e));
  gen::RefillArgs r;
  r.E = p->num_envs; r.W = cs->window; r.env_id_offset = ar->env_id_offset;
  r.reset_count = s->reset_count; r.held = cs->held; r.seen = cs->seen;
  r.work_index = reinterpret_cast<long long*>(cs->work_index); r.work_row = reinterpret_cast<long long*>(cs->work_row);
  r.work_count = cs->work_count;
  if (const int rl = launch(gen::stream_refill_kernel, dim3(static_cast<unsigned>((rows + 255) / 256)), dim3(256), 0, st, r)) return rl;
  return launch_generate_at(a, cs->work_index, cs->work_row, cs->work_count, rows, stream);
}

int cagpu_generate_cases(int64_t num_cases, int32_t num_agents, double side_lo, double side_hi, double speed_lo,
                         double speed_hi, double radius_lo, double radius_hi, uint64_t seed, double* cases, int32_t* status,
                         void* stream) {
  return generate_impl(num_cases, num_agents, 0, 0, nullptr, 0, side_lo, side_hi, speed_lo, speed_hi, radius_lo, radius_hi,
                       seed, cases, nullptr, status, stream);
}

int cagpu_generate_cases_ragged(int64_t num_cases, int32_t max_agents, int32_t n_min, int32_t n_max,
                                const double* side_ranges, int32_t n_ranges, double speed_lo, double speed_hi,
                                double radius_lo, double radius_hi, uint64_t seed, double* cases, int32_t* counts,
                                int32_t* status, void* stream) {
  if (n_ranges < 1) return fail(CA_EINVAL, "cagpu_generate_cases_ragged: need at least one side range%s");
  if (n_max < 1) return fail(CA_EINVAL, "cagpu_generate_cases_ragged: need 1 <= n_min <= n_max <= max_agents%s");
  return generate_impl(num_cases, max_agents, n_min, n_max, side_ranges, n_ranges, 1.0, 1.0, speed_lo, speed_hi, radius_lo,
                       radius_hi, seed, cases, counts, status, stream);
}

int cagpu_rollout(const CaParams* p, const CaState* s, const CaOut* o, const double* ext_actions, const CaAutoReset* ar,
                  int32_t n_steps, void* stream) {
  StepCall c;
  c.who = "cagpu_rollout"; c.n_steps = n_steps;
  return step_impl(p, s, o, ext_actions, ar, c, stream);
}

int cagpu_rollout_ring(const CaParams* p, const CaState* s, const CaOut* o, const double* ext_actions, const CaAutoReset* ar,
                       int32_t n_steps, int64_t snapshot_delta, void* stream) {
  StepCall c;
  c.who = "cagpu_rollout_ring"; c.n_steps = n_steps; c.ring = true; c.snapshot_delta = snapshot_delta;
  return step_impl(p, s, o, ext_actions, ar, c, stream);
}

int cagpu_ring_snapshots(const CaParams* p, const CaState* s, const CaOut* o, const CaAutoReset* ar, int32_t n_steps) {
  StepCall c;
  c.who = "cagpu_ring_snapshots"; c.n_steps = n_steps; c.ring = true; c.query_snapshot = true;
  return step_impl(p, s, o, nullptr, ar, c, nullptr);
}

int cagpu_plan(const CaParams* p, const CaState* s, void* stream) {
  if (!p || !s) return fail(CA_EINVAL, "cagpu_plan: NULL params/state%s");
  if (p->num_agents > 10) return fail(CA_EUNSUPPORTED, "cagpu_plan: no pipelined step kernel for more than 10 agents per env%s");
  CaOut o;
  std::memset(&o, 0, sizeof(o));
  o.obs = reinterpret_cast<float*>(1); o.rewards = o.obs; o.done = reinterpret_cast<uint8_t*>(1); o.game_over = o.done;  // (not touched in this mode)
  int rc = check_params(p, s, &o);
  if (rc) return rc;
  if (!s->next_action) return fail(CA_EINVAL, "cagpu_plan: CaState.next_action is NULL%s");
  KArgs k;
  std::memset(&k, 0, sizeof(k));
  k.p = *p; k.s = *s;
  k.n_steps = 1; k.mode = pipe::MODE_PLAN;
  k.inv_rvo_dt = 1.0 / p->rvo_dt;
  return launch_any(k, stream);
}

int cagpu_observe(const CaParams* p, const CaState* s, const CaOut* o, void* stream) {
  int rc = check_params(p, s, o);
  if (rc) return rc;
  KArgs k;
  std::memset(&k, 0, sizeof(k));
  k.p = *p; k.s = *s; k.o = *o;
  k.n_steps = 1; k.mode = MODE_OBSERVE;
  return launch_any(k, stream);
}


uint64_t cagpu_ga3c_packed_bytes(void) { return static_cast<uint64_t>(ga3c::PK_TOTAL) * sizeof(ga3c::u32x4); }

int cagpu_ga3c_pack(const CaNet* net, void* packed, uint64_t bytes, void* stream) {
  if (!net || !packed) return fail(CA_EINVAL, "cagpu_ga3c_pack: NULL argument%s");
  if (bytes < cagpu_ga3c_packed_bytes() || (reinterpret_cast<uintptr_t>(packed) & 15))
    return fail(CA_EINVAL, "cagpu_ga3c_pack: the buffer must hold cagpu_ga3c_packed_bytes() bytes, 16-byte aligned%s");
  if (!net->lstm_kernel || !net->layer1_kernel || !net->layer2_kernel || !net->fc1_kernel)
    return fail(CA_EINVAL, "cagpu_ga3c_pack: NULL weight pointer%s");
  ga3c::u32x4* out = static_cast<ga3c::u32x4*>(packed);
  struct { const float* w; int row0, k_real, nkb, at; } jobs[4] = {
      {net->lstm_kernel, 7, 64, 2, ga3c::PK_LSTM},     // rows 0..6 (x_t) and the bias: split by the kernel itself
      {net->layer1_kernel, 4, 64, 2, ga3c::PK_L1},     // rows 0..3 (host) stay float32
      {net->layer2_kernel, 0, 256, 8, ga3c::PK_L2},
      {net->fc1_kernel, 0, 256, 8, ga3c::PK_FC1}};
  for (const auto& j : jobs) {
    const int threads = j.nkb * 16 * 64;
    hipLaunchKernelGGL(ga3c::pack_kernel, dim3((threads + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), j.w,
                       j.row0, j.k_real, j.nkb, out + j.at, j.at == ga3c::PK_LSTM ? 1 : 0);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(CA_ELAUNCH, "cagpu_ga3c_pack: kernel launch failed: %s", hipGetErrorString(e));
  return CA_OK;
}

uint64_t cagpu_workspace_bytes(const CaParams* p) {
  if (!p || p->num_agents <= 64 || p->num_agents > big::NT_MAX || p->num_envs < 1) return 0;
  // two resident workgroups per CU keep the device busy (one above 256 agents: 8 / 16 waves and up to 88 KB of LDS each);
  // more only cost memory (a share is 15 MB at 512 agents, 63 MB at 1024)
  long wgs = (p->num_agents <= 256 ? 2L : 1L) * device_cus();
  if (wgs < 1) wgs = 512;
  if (wgs > p->num_envs) wgs = p->num_envs;
  return static_cast<uint64_t>(wgs) * big::ws_bytes_per_wg(p->num_agents);
}

int cagpu_device_faults(uint32_t* faults, int32_t clear) {
  if (!faults) return fail(CA_EINVAL, "cagpu_device_faults: NULL pointer%s");
  unsigned int v = 0u;
  hipError_t e = hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_fault), sizeof(v));  // (synchronises the device)
  if (e == hipSuccess && clear && v) {
    const unsigned int z = 0u;
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_fault), &z, sizeof(z));
  }
  if (e != hipSuccess) return fail(CA_ELAUNCH, "cagpu_device_faults: %s", hipGetErrorString(e));
  *faults = v;
  return CA_OK;
}

int cagpu_device_faults_async(uint32_t* host_dst, void* stream) {
  if (!host_dst) return fail(CA_EINVAL, "cagpu_device_faults_async: NULL pointer%s");
  hipError_t e = hipMemcpyFromSymbolAsync(host_dst, HIP_SYMBOL(g_fault), sizeof(unsigned int), 0, hipMemcpyDeviceToHost,
                                          static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(CA_ELAUNCH, "cagpu_device_faults_async: %s", hipGetErrorString(e));
  return CA_OK;
}

int cagpu_debug_libm(int32_t op, int32_t n, const double* a, const double* b, double* out0, double* out1) {
  if (n < 1 || !a || !out0 || op < 0 || op > 6) return fail(CA_EINVAL, "cagpu_debug_libm: bad arguments%s");
  double* d = nullptr;
  const size_t sz = sizeof(double) * static_cast<size_t>(n);
  if (hipMalloc(reinterpret_cast<void**>(&d), 4 * sz) != hipSuccess) return fail(CA_ELAUNCH, "cagpu_debug_libm: hipMalloc failed%s");
  hipError_t e = hipMemcpy(d, a, sz, hipMemcpyHostToDevice);
  if (e == hipSuccess && b) e = hipMemcpy(d + n, b, sz, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(debug_libm_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, n, op, d, b ? d + n : nullptr, d + 2 * n,
                       d + 3 * n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out0, d + 2 * n, sz, hipMemcpyDeviceToHost);
  if (e == hipSuccess && out1) e = hipMemcpy(out1, d + 3 * n, sz, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(CA_ELAUNCH, "cagpu_debug_libm: %s", hipGetErrorString(e));
  return CA_OK;
}

int cagpu_debug_copy8(int64_t n, const double* src, double* dst, void* stream) {
  if (n < 1 || !src || !dst) return fail(CA_EINVAL, "cagpu_debug_copy8: bad arguments%s");
  return launch(copy8_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                static_cast<long>(n), src, dst);
}

uint64_t cagpu_episode_metrics_carry_bytes(const CaParams* p) {
  if (!p || p->num_envs < 1 || p->num_agents < 1 || p->num_agents > 1024) return 0;
  return static_cast<uint64_t>(p->num_envs) * metrics_carry_env_bytes(p->num_agents);
}

int cagpu_episode_metrics(const CaParams* p, const CaTraj* traj, int32_t n_steps, const CaEpMetrics* m, void* stream) {
  if (!p || !traj || !m) return fail(CA_EINVAL, "cagpu_episode_metrics: NULL argument%s");
  if (p->num_envs < 1 || p->num_agents < 1 || p->num_agents > 1024) return fail(CA_EINVAL, "cagpu_episode_metrics: bad sizes%s");
  const auto bad = [](const void* q, uintptr_t mask) { return !q || (reinterpret_cast<uintptr_t>(q) & mask); };
  if (bad(traj->rows, 15) || bad(traj->episode, 3))
    return fail(CA_EINVAL, "cagpu_episode_metrics: traj->rows NULL or not 16-byte aligned, or traj->episode NULL or not 4-byte aligned%s");
  if (bad(m->vals, 15) || bad(m->cnts, 15) || bad(m->head, 3) || bad(m->carry, 15))
    return fail(CA_EINVAL, "cagpu_episode_metrics: vals / cnts / carry NULL or not 16-byte aligned, or head NULL or not 4-byte aligned%s");
  if (m->capacity < 1) return fail(CA_EINVAL, "cagpu_episode_metrics: capacity < 1%s");
  if (n_steps < 0) return fail(CA_EINVAL, "cagpu_episode_metrics: n_steps < 0%s");
  if (n_steps == 0) return CA_OK;
  MetricsArgs k;
  k.rows = traj->rows; k.episode = traj->episode;
  k.vals = m->vals; k.cnts = m->cnts; k.head = m->head; k.carry = static_cast<unsigned char*>(m->carry);
  k.E = p->num_envs; k.N = p->num_agents; k.T = n_steps; k.C = m->capacity;
  k.dt = p->dt; k.close_range = m->getting_close_range;
  const int nt = (p->num_agents + 63) & ~63;
  const size_t lds = static_cast<size_t>(nt) * 28;
  if (const int rc = launch(nt == 64 ? &metrics_kernel<64> : &metrics_kernel<1024>, dim3(static_cast<unsigned>(k.E)), dim3(nt), lds,
                            static_cast<hipStream_t>(stream), k))
    return rc;
  std::snprintf(g_last_kernel, sizeof(g_last_kernel), "metrics_kernel<%d> grid=%d threads=%d lds=%zu steps=%d", nt == 64 ? 64 : 1024,
                k.E, nt, lds, n_steps);
  return CA_OK;
}

int cagpu_orca(int32_t num_envs, int32_t num_agents, const float* pos, const float* vel, const float* pref,
               const float* radius, const float* max_speed, float collab_coeff, float time_horizon, float time_step,
               int32_t max_neighbors, float neighbor_dist, float* new_vel, void* stream) {
  if (num_envs < 1 || num_agents < 1) return fail(CA_EINVAL, "cagpu_orca: bad sizes%s");
  if (num_agents > 64) return fail(CA_EUNSUPPORTED, "cagpu_orca: num_agents > 64 not supported yet%s");
  if (!pos || !vel || !pref || !radius || !max_speed || !new_vel) return fail(CA_EINVAL, "cagpu_orca: NULL pointer%s");
  OrcaArgs k;
  k.num_envs = num_envs; k.num_agents = num_agents; k.max_nb = max_neighbors;
  k.pos = pos; k.vel = vel; k.pref = pref; k.radius = radius; k.max_speed = max_speed;
  k.collab = collab_coeff; k.time_horizon = time_horizon; k.time_step = time_step; k.neighbor_dist = neighbor_dist;
  k.new_vel = new_vel;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (pick_block(num_agents)) {
    case 64: return launch_orca<64>(k, st);
    case 128: return launch_orca<128>(k, st);
    default: return launch_orca<256>(k, st);
  }
}

// ---- map sensors for every step of a fused launch (csrc/cagpu_poses.inc)
static bool bad_ptr(const void* q, uintptr_t mask) { return !q || (reinterpret_cast<uintptr_t>(q) & mask); }

static int check_pose_ring(const CaPoseRing* r, const bool need_map, const char* who) {
  if (!r) return fail(CA_EINVAL, "%s: NULL CaPoseRing", who);
  if (bad_ptr(r->pos_x, 15) || bad_ptr(r->pos_y, 15) || bad_ptr(r->heading, 15) || bad_ptr(r->radius, 15) ||
      bad_ptr(r->step_num, 15))
    return fail(CA_EINVAL, "%s: a CaPoseRing array is NULL or not 16-byte aligned", who);
  if (need_map ? bad_ptr(r->env_map, 3) : (reinterpret_cast<uintptr_t>(r->env_map) & 3) != 0)
    return fail(CA_EINVAL, "%s: CaPoseRing.env_map NULL with a map set, or not 4-byte aligned", who);
  return CA_OK;
}

int cagpu_tape_poses(const CaParams* p, const CaState* start, const int32_t* start_env_map, const CaTraj* traj,
                     const uint8_t* game_over, int32_t n_steps, const CaAutoReset* ar, const CaMapSet* set,
                     const CaPoseRing* ring, void* stream) {
  const char* who = "cagpu_tape_poses";
  if (!p || !start || !traj || !game_over || !ring) return fail(CA_EINVAL, "%s: NULL argument", who);
  if (p->num_envs < 1 || p->num_agents < 1 || p->num_agents > big::NT_MAX) return fail(CA_EINVAL, "%s: bad sizes", who);
  if (n_steps < 0) return fail(CA_EINVAL, "%s: n_steps < 0", who);
  if (!start->pos_x || !start->pos_y || !start->heading || !start->radius || !start->step_num || !start->reset_count)
    return fail(CA_EINVAL, "%s: NULL state pointer", who);
  if (bad_ptr(traj->rows, 15)) return fail(CA_EINVAL, "%s: traj->rows NULL or not 16-byte aligned", who);
  if (set) {
    if (set->num_maps < 1) return fail(CA_EINVAL, "%s: CaMapSet.num_maps < 1", who);
    if (bad_ptr(start_env_map, 3)) return fail(CA_EINVAL, "%s: start_env_map NULL or not 4-byte aligned with a map set", who);
  }
  if (ar && (!ar->table || ar->n_cases < 1)) return fail(CA_EINVAL, "%s: bad CaAutoReset", who);
  const int rc = check_pose_ring(ring, set != nullptr, who);
  if (rc) return rc;
  if (n_steps == 0) return CA_OK;
  PoseArgs k;
  std::memset(&k, 0, sizeof(k));
  k.p = *p;
  k.pos_x = start->pos_x; k.pos_y = start->pos_y; k.heading = start->heading; k.radius = start->radius;
  k.step_num = start->step_num; k.reset_count = start->reset_count;
  k.env_map_in = set ? start_env_map : nullptr;
  k.rows = traj->rows; k.game_over = game_over; k.n_steps = n_steps;
  if (ar) {
    k.table = ar->table; k.n_cases = ar->n_cases; k.env_id_offset = ar->env_id_offset; k.case_stride = ar->case_stride;
    k.heading_seed = ar->heading_seed;
    if (set) { k.map_seed = set->map_seed; k.num_maps = set->num_maps; }
  }
  k.o_px = ring->pos_x; k.o_py = ring->pos_y; k.o_hd = ring->heading; k.o_rad = ring->radius;
  k.o_step = ring->step_num; k.o_map = set ? ring->env_map : nullptr;
  const long EN = static_cast<long>(p->num_envs) * p->num_agents;
  return launch(poses_kernel, dim3(static_cast<unsigned>((EN + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), k);
}

int cagpu_laserscan_slots(const CaParams* p, const CaPoseRing* ring, int32_t n_steps, const CaMap* map, const CaMapSet* set,
                          const CaScan* scan, uint8_t* idx, void* stream) {
  const char* who = "cagpu_laserscan_slots";
  if (!p || !ring || !scan || (!map && !set)) return fail(CA_EINVAL, "%s: NULL argument", who);
  if (map && set) return fail(CA_EINVAL, "%s: map and set at once", who);
  if (p->num_envs < 1 || p->num_agents < 1) return fail(CA_EINVAL, "%s: bad sizes", who);
  if (n_steps < 0) return fail(CA_EINVAL, "%s: n_steps < 0", who);
  if (static_cast<long>(n_steps) * p->num_envs > 0x7FFFFFFFL) return fail(CA_EUNSUPPORTED, "%s: more than 2^31 - 1 (slot, env) pairs", who);
  if (bad_ptr(idx, 15)) return fail(CA_EINVAL, "%s: idx NULL or not 16-byte aligned", who);
  if (set && (!set->map.static_bits || set->num_maps < 1)) return fail(CA_EINVAL, "%s: bad CaMapSet", who);
  const int rc = check_pose_ring(ring, set != nullptr, who);
  if (rc) return rc;
  if (n_steps == 0) return CA_OK;
  CaParams pp = *p;
  pp.num_envs = p->num_envs * n_steps;  // the ring is [n, E, N]: n x E envs of N agents
  CaState s;
  std::memset(&s, 0, sizeof(s));
  s.pos_x = ring->pos_x; s.pos_y = ring->pos_y; s.heading = ring->heading; s.radius = ring->radius; s.step_num = ring->step_num;
  if (set) {
    CaMapSet ms = *set;
    ms.env_map = ring->env_map;
    return laserscan_impl(&pp, &s, &ms.map, scan, stream, &ms, idx);
  }
  return laserscan_impl(&pp, &s, map, scan, stream, nullptr, idx);
}

int cagpu_laserscan_history(const CaParams* p, const CaScan* scan, const uint8_t* idx, const int32_t* step_num, int32_t n_steps,
                            int32_t first, int32_t count, uint8_t* hist_out, float* out, void* stream) {
  const char* who = "cagpu_laserscan_history";
  if (!p || !scan) return fail(CA_EINVAL, "%s: NULL argument", who);
  if (p->num_envs < 1 || p->num_agents < 1) return fail(CA_EINVAL, "%s: bad sizes", who);
  if (scan->num_beams < 2 || scan->num_to_store < 1 || scan->num_ranges < 1 || scan->num_ranges > 255)
    return fail(CA_EINVAL, "%s: bad CaScan", who);
  if (n_steps < 1 || first < 0 || count < 0 || first > n_steps - count)
    return fail(CA_EINVAL, "%s: n_steps < 1 or [first, first + count) outside the n_steps slots", who);
  if (bad_ptr(idx, 15) || bad_ptr(step_num, 15) || bad_ptr(scan->hist, 15))
    return fail(CA_EINVAL, "%s: idx, step_num or CaScan.hist NULL or not 16-byte aligned", who);
  if ((!hist_out && !out) || ((reinterpret_cast<uintptr_t>(hist_out) | reinterpret_cast<uintptr_t>(out)) & 15))
    return fail(CA_EINVAL, "%s: both outputs NULL, or an output not 16-byte aligned", who);
  if (hist_out == scan->hist && count != 1)
    return fail(CA_EINVAL, "%s: only a single slot may be expanded in place (hist_out == CaScan.hist)", who);
  if (count == 0) return CA_OK;
  ScanHistArgs k;
  std::memset(&k, 0, sizeof(k));
  k.idx = idx; k.step_num = step_num; k.carried = scan->hist; k.o_hist = hist_out; k.o_out = out;
  k.EN = static_cast<long>(p->num_envs) * p->num_agents;
  k.first = first; k.count = count; k.B = scan->num_beams; k.H = scan->num_to_store;
  k.range_res = scan->range_res; k.max_range = scan->max_range;
  const bool vec = (k.B & 3) == 0;
  const long threads = k.EN * (vec ? k.B / 4 : k.B) * count;
  if ((threads + 255) / 256 > 0x7FFFFFFFL) return fail(CA_EUNSUPPORTED, "%s: too many (slot, agent, beam) items for one launch", who);
  const dim3 grid(static_cast<unsigned>((threads + 255) / 256));
  return launch(vec ? &scan_hist_kernel<4> : &scan_hist_kernel<1>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), k);
}

}  // extern "C"
