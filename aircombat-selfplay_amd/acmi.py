"""Tacview ACMI text records of one env: the format written by BaseEnv.render (envs/JSBSim/envs/env_base.py:207-250)
from BaseSimulator.log / MissileSimulator.log (core/simulatior.py:73-79, 535-551). Host-side only; not on the step() path."""
import math

HEADER = "FileType=text/acmi/tacview\nFileVersion=2.1\n0,ReferenceTime=2020-04-01T00:00:00Z\n"
_A, _F = 6378137.0, 1 / 298.257223563
_B = _A * (1 - _F)


def neu_to_lla(n, e, u, lon0, lat0, alt0):
    """NEU2LLA (utils/utils.py:44-55 -> pymap3d.ned2geodetic): ENU offset about the battle-field centre -> lon, lat (deg), height (m).
    Geodetic -> ECEF, rotate the offset into ECEF, then the closed-form inverse (Bowring start + two Newton steps: < 1e-9 deg)."""
    la0, lo0 = math.radians(lat0), math.radians(lon0)
    N0 = _A ** 2 / math.hypot(_A * math.cos(la0), _B * math.sin(la0))
    x0 = (N0 + alt0) * math.cos(la0) * math.cos(lo0)
    y0 = (N0 + alt0) * math.cos(la0) * math.sin(lo0)
    z0 = (N0 * (_B / _A) ** 2 + alt0) * math.sin(la0)
    t = math.cos(la0) * u - math.sin(la0) * n
    x = x0 + math.cos(lo0) * t - math.sin(lo0) * e
    y = y0 + math.sin(lo0) * t + math.cos(lo0) * e
    z = z0 + math.sin(la0) * u + math.cos(la0) * n
    e2 = 1 - (_B / _A) ** 2
    p = math.hypot(x, y)
    lat = math.atan2(z, p * (1 - e2))
    for _ in range(4):
        Nn = _A / math.sqrt(1 - e2 * math.sin(lat) ** 2)
        h = p / math.cos(lat) - Nn
        lat = math.atan2(z, p * (1 - e2 * Nn / (Nn + h)))
    Nn = _A / math.sqrt(1 - e2 * math.sin(lat) ** 2)
    return math.degrees(math.atan2(y, x)), math.degrees(lat), p / math.cos(lat) - Nn


MISSILE_MODELS = {0: "AIM-9L", 1: "AIM-120B", 2: "AIM-9M"}   # ac_get_missile's model code -> MissileSimulator.model


def aircraft_record(uid, color, entity, model="f16"):
    """BaseSimulator.log (simulatior.py:73-79): `entity` = ac_get_entity's lon, lat (deg), alt (m), roll, pitch, yaw (rad), ..."""
    lon, lat, alt, roll, pitch, yaw = entity[:6]
    deg = lambda x: x * 180 / math.pi           # get_rpy() * 180 / np.pi, in the reference's operation order
    return (f"{uid},T={lon}|{lat}|{alt}|{deg(roll)}|{deg(pitch)}|{deg(yaw)},"
            f"Name={model.upper()},Color={color}")


def missile_records(uid, color, status, neu, theta, psi, center, exploded, radius, model="AIM-9L"):
    """MissileSimulator.log (simulatior.py:535-551): alive -> a position record; first frame after it is done -> removal + explosion;
    later -> removal (the reference's removal message carries its own newline, so the file shows an empty line after it).
    Returns (text, exploded_flag)."""
    lon, lat, alt = neu_to_lla(neu[0], neu[1], neu[2], *center)
    pose = f"T={lon}|{lat}|{alt}|0.0|{theta * 180 / math.pi}|{psi * 180 / math.pi}"
    if status == 0:
        return f"{uid},{pose},Name={model.upper()},Color={color}", exploded
    if not exploded:
        return f"-{uid}\n{uid}F,{pose},Type=Misc+Explosion,Color={color},Radius={radius}", True
    return f"-{uid}\n", exploded


def chaff_record(uid, color, alive, pose, model="CHF"):
    """ChaffSimulator.log (simulatior.py:383-388): the cloud keeps the geodetic position and attitude its parent had at the release
    (`pose` = lon, lat, alt, roll, pitch, yaw) while it is effective; afterwards the removal message."""
    if alive:
        return aircraft_record(uid, color, pose, model)
    return f"-{uid}\n"


def chaff_from_words(w0, w1):
    """The chaff bookkeeping inside the scenario tasks' two packed extension words (csrc/scenario_kernel.hpp: n_ch in bits 2-3 of the
    second word, the clouds' status bits 4 and 5, their multiplicities bits 6-10 and 11-15): (n_ch, ((status0, mult0), (status1, mult1)))."""
    w1 = int(w1)
    return (w1 >> 2) & 3, (((w1 >> 4) & 1, (w1 >> 6) & 31), ((w1 >> 5) & 1, (w1 >> 11) & 31))


class FrameWriter:
    """BaseEnv.render's bookkeeping for one env (env_base.py:207-250), one frame at a time: which munitions have shown their explosion
    record (MissileSimulator.log writes it once), the order of env._tempsims (a uid keeps the dict position of its first launch), the
    chaff clouds of env._chaffsims with the pose their parent had at the release, and env.reset() clearing all of it, seen as a
    `cur_step` that does not increase. ``HipVecEnv.render`` feeds it from the host getters and ``FlightRecorder.write_acmi`` from
    recorded frames; the text is the same because this is the only place that writes it.

    ``frame(cur_step, entities, slots, chaff)`` returns the frame's text ('#time' line and one record per line):
      entities[a]   ac_get_entity's values of aircraft a (at least the first six)
      slots[a][k]   (status, model, px, py, pz, theta, psi) of munition slot k, model = ac_get_missile's out[11]; read for the slots
                    the task's uids cover (the 1v1 missile tasks: min(num_missiles, 4); the scenario family: 2)
      chaff[a]      (n_ch, ((status0, mult0), (status1, mult1))), see chaff_from_words; read for the scenario tasks only"""

    def __init__(self, cfg, num_agents=None):
        self.cfg = cfg
        self.num_agents = int(num_agents if num_agents is not None else cfg.n_agents)
        A, ne = self.num_agents, int(cfg.n_ego)
        self.center = (cfg.center_lon, cfg.center_lat, cfg.center_alt)
        self.uids = getattr(cfg, "uids", None) or [f"{'A' if a < ne else 'B'}0{(a if a < ne else a - ne) + 1}00" for a in range(A)]
        self.colors = ["Blue" if a < ne else "Red" for a in range(A)]
        task = int(cfg.task)
        slots = {3: 4, 2: 4, 5: 2, 6: 2}.get(task, 0)          # AC_TASK_SHOOT_MISSILE, _DODGE_MISSILE, _SCENARIO1, _SCENARIO_NVN
        self.radius = 300 if task in (3, 2) else 5             # MissileSimulator itself (300 m fuse) against the scenario munitions' 5 m
        if task == 2 and int(cfg.n_agents) > 2:                # multiplecombat_dodge_missile: two uids per aircraft, like the scenario tasks
            slots = 2
        # a slot's uid is "agent + remaining count at the launch" (scenario1_task.py:83,92; singlecombat_with_missile_task.py:199): slots
        # are consumed from the highest count down
        self.n_slots = [min(int(cfg.num_missiles[a]), slots) if slots == 4 else slots for a in range(A)]
        self.has_chaff = task in (5, 6)
        self.last_step = -1
        self.clear()

    def clear(self):
        self.exploded, self.first, self.chaff = set(), {}, {}

    def frame(self, cur_step, entities, slots=None, chaff=None):
        step = int(cur_step)
        if step <= self.last_step:      # the episode was reset: env.reset() clears _tempsims / _chaffsims (env_base.py:98-113)
            self.clear()
        self.last_step = step
        A, uids, colors = self.num_agents, self.uids, self.colors
        msgs = [aircraft_record(uids[a], colors[a], entities[a]) for a in range(A)]
        # env._tempsims in dict order = first-launch order of the uids
        flying = []
        for a in range(A):
            for k in range(self.n_slots[a]):
                m = slots[a][k]
                if m[0] < 0:
                    self.exploded.discard((a, k))
                    continue
                flying.append((a, k, m))
        for a, k, _m in flying:
            self.first.setdefault((a, k), (step, a))      # dict position of the uid: its first launch (step, agent order)
        flying.sort(key=lambda r: self.first[(r[0], r[1])])
        for a, k, m in flying:
            uid = f"{uids[a]}{self.n_slots[a] - k}"
            rec, boom = missile_records(uid, colors[a], int(m[0]), m[2:5], m[5], m[6], self.center, (a, k) in self.exploded,
                                        self.radius, MISSILE_MODELS[int(m[1])])
            if boom:
                self.exploded.add((a, k))
            msgs.append(rec)
        # env._chaffsims: one ChaffSimulator per qualifying incoming missile of a release event, uid "agent + (remaining + 10)"
        if self.has_chaff:
            for a in range(A):
                n_ch, clouds = chaff[a]
                rem = int(self.cfg.num_missiles[a])
                for q in range(min(int(n_ch), 2)):
                    status, mult = clouds[q]
                    for _ in range(int(mult)):
                        uid = f"{uids[a]}{rem + 10}"
                        rem -= 1
                        if uid not in self.chaff:
                            self.chaff[uid] = {"color": colors[a], "pose": tuple(entities[a][:6])}
                        self.chaff[uid]["alive"] = int(status) == 0
            for uid, ch in self.chaff.items():
                msgs.append(chaff_record(uid, ch["color"], ch["alive"], ch["pose"]))
        return f"#{step * self.cfg.agent_interaction_steps / self.cfg.sim_freq:.2f}\n" + "".join(msg + "\n" for msg in msgs)
