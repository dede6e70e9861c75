// uavx_multi.hip — E x MultiUAVWorld2D on one MI355X: fused step / reset / observe kernels and the
// C ABI of include/uavx.h.  Hand-written for gfx950 (wave64, LDS-staged neighbour exchange).
//
// Reference semantics (cited per block): MUW = gym_uav_collision_avoidance/envs/multi_uav_world_2d.py,
// AG = .../uav_agent.py of dazchi/gym-uav-collision-avoidance.
//
// Work mapping.  One LANE per agent, floor(64/N) whole envs per WAVEFRONT, one wavefront per workgroup, so that all
// cross-agent traffic of an env stays inside its wave (agent counts that would leave many lanes of one wavefront idle use
// workgroups of 2..4 wavefronts instead, pick_group_waves(): an env may then span two waves of ONE workgroup, and the
// wave-local ordering points below become workgroup barriers):
//   1. every lane integrates its own agent (float64 velocity, float32 position, AG:23-36) — the
//      reference's sequential loop over agents (MUW:181) has no real dependency here because an
//      agent's motion only reads its own state;
//   2. old + new position and heading of every agent are staged in LDS (20 B per lane);
//   3. every lane scans the N-1 other agents of its env from LDS: the Gauss-Seidel rule "agents
//      j<i already moved, j>i not yet" (MUW:181-231) becomes a per-pair select between the staged
//      new/old position; min-distance feeds the collision tests, the two nearest at final positions
//      feed the observation (AG:44-64, MUW:75-95);
//   4. reward / collision / termination / finish() per lane (MUW:188-231, AG:38-42);
//   5. the 10 observation floats per agent are transposed through LDS so the wave writes its
//      2560-byte obs block with 16-byte-per-lane contiguous stores.
// HBM layout (agent slot a = e*N + i, agent fastest => lane-contiguous):
//   pos  float2[A]  {x, y}                     read+write    8 B
//   vel  double2[A] {vx, vy}                   read+write   16 B
//   goal float4[A]  {tx, ty, init_d, flags}    read         16 B   (flags word rewritten only when it changes)
//   prev_distance (AG:18) is NOT stored: for an agent that is not done it always equals ||target - location||
//   (AG:33-34, MUW:155,229), so it is recomputed from the loaded position; values a caller pokes in that
//   break this identity live in prev_ovr[A] behind the PREVD_OVR flag bit (read only when the bit is set).
//   per workgroup: wave_steps[G] (one no-return atomic per launch; env.steps = wave_steps - env_rec.x)
//   per env:   reach[E] / coll[E] (atomics on the rare events), env_rec[E] (16 B: steps base, episode index,
//              running returns; touched by reset / step_ex only), episode statistics (fin_*).
// Kernel arguments: the step kernels take what their FIRST instructions need as leading scalars (command pointer, base of the
// state allocation + 32-bit array offsets, the numbers of the lane mapping), which gfx950 preloads into SGPRs with the wavefront
// (Makefile: -mllvm -amdgpu-kernarg-preload-count), and everything else in the by-value MultiParams behind them: the state loads
// are the first thing a wavefront does (step_kernel, step_ex_kernel; profiles/r04_ab_notes.md section 10).
// BASELINE configs[4] extension (scripted bodies, per-env curriculum levels; EXT kernel variants): see MultiParams and
// include/uavx.h; lanes stay one per LEARNER there and the bodies are extra rows of the env's LDS neighbour tile.
// A body is a position (float2, read + written while it moves) and a leg record {dx, dy, heading, legs} (float4, read
// only between two waypoint changes): 24 B read + 8 B written per body-step, two float32 additions of arithmetic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>

#include "../../include/uavx.h"
#include "uavx_device.hpp"

namespace uavx {
#include "uavx_multi_params.hpp"
#include "uavx_multi_scan.hpp"
#include "uavx_multi_step.hpp"
#include "uavx_multi_reset.hpp"
#include "uavx_multi_kernels.hpp"
}  // namespace uavx

// ------------------------------------------------------------------------------------------------
// host side: handle + C ABI
// ------------------------------------------------------------------------------------------------
using namespace uavx;

#include "uavx_host_util.hpp"
#include "uavx_multi_handle.hpp"
#include "uavx_multi_launch.hpp"
#include "uavx_multi_host.hpp"
#include "uavx_multi_snapshot.hpp"
