// Launch recorder: stands in for the HIP runtime entry points the library launches through.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include <cxxabi.h>

static std::map<const void*, std::string>& names()
{
    static std::map<const void*, std::string> m;
    return m;
}
static std::string g_log;
struct Cfg { dim3 g, b; size_t lds; hipStream_t st; };
static thread_local std::vector<Cfg> g_stack;
// rec_mode (record_gto.py; record.py leaves all three off)
enum { REC_DEVICE = 1,      // hipGetDevice answers device 0: the library's internal stream and events exist
       REC_COPY = 2,        // a device-to-host hipMemcpyAsync really copies (the "device" pointer is a host array)
       REC_STREAMS = 4 };   // a launch says whether its stream is the caller's; event records and waits are logged
static int g_mode = 0;
static hipStream_t g_caller = nullptr;
static char g_streams[4], g_events[256];         // what the stand-ins hand out pointers to
static int g_nstream = 0, g_nevent = 0;

static const char* stream_name(hipStream_t st) { return st == g_caller ? "caller" : "internal"; }
static void log_event(const char* what, hipEvent_t ev, hipStream_t st)
{
    if (!(g_mode & REC_STREAMS)) return;
    char buf[96];
    snprintf(buf, sizeof buf, "%s event %d %s\n", what, (int)(reinterpret_cast<char*>(ev) - g_events), stream_name(st));
    g_log += buf;
}

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* dummy[4]; return dummy; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* hostFunction, char*, const char* deviceName, unsigned, void*, void*,
                           dim3*, dim3*, int*)
{
    int status = 0;
    char* d = abi::__cxa_demangle(deviceName, nullptr, nullptr, &status);
    names()[hostFunction] = (status == 0 && d) ? d : deviceName;
    free(d);
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t lds, hipStream_t st)
{
    g_stack.push_back(Cfg{g, b, lds, st});
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* lds, hipStream_t* st)
{
    Cfg c = g_stack.back();
    g_stack.pop_back();
    *g = c.g; *b = c.b; *lds = c.lds; *st = c.st;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void**, size_t lds, hipStream_t st)
{
    std::string n = names().count(f) ? names()[f] : "?";
    // strip the argument list and the anonymous namespace
    size_t p = n.find("(anonymous namespace)::");
    if (p != std::string::npos) n.erase(p, 23);
    if (n.compare(0, 5, "void ") == 0) n.erase(0, 5);
    int depth = 0;
    for (size_t i = 0; i < n.size(); ++i) {
        if (n[i] == '<') ++depth;
        else if (n[i] == '>') --depth;
        else if (n[i] == '(' && depth == 0) { n.erase(i); break; }
    }
    char buf[128];
    snprintf(buf, sizeof buf, " grid=%u,%u,%u block=%u lds=%zu", g.x, g.y, g.z, b.x, lds);
    g_log += n + buf;
    if (g_mode & REC_STREAMS) g_log += std::string(" stream=") + stream_name(st);
    g_log += "\n";
    return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipGetDevice(int* dev)
{
    if (!(g_mode & REC_DEVICE)) return hipErrorNoDevice;
    *dev = 0;
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* st, unsigned)
{
    if (g_nstream >= (int)sizeof g_streams) return hipErrorOutOfMemory;
    *st = reinterpret_cast<hipStream_t>(&g_streams[g_nstream++]);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned)
{
    if (g_nevent >= (int)sizeof g_events) return hipErrorOutOfMemory;
    *ev = reinterpret_cast<hipEvent_t>(&g_events[g_nevent++]);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t st) { log_event("record", ev, st); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t ev, unsigned) { log_event("wait", ev, st); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t st)
{
    if (g_mode & REC_STREAMS) g_log += std::string("synchronize ") + stream_name(st) + "\n";
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t)
{
    g_log += "memcpy\n";
    if ((g_mode & REC_COPY) && kind == hipMemcpyDeviceToHost) memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int* n, const void*, int, size_t) { *n = 1; return hipSuccess; }
void rec_reset(void) { g_log.clear(); }
const char* rec_log(void) { return g_log.c_str(); }
void rec_mode(int mode, void* caller_stream) { g_mode = mode; g_caller = (hipStream_t)caller_stream; }
}
