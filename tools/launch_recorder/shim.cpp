// Launch recorder: stands in for the HIP runtime entry points the library launches through.
#include <hip/hip_runtime.h>
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
hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void**, size_t lds, hipStream_t)
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
    snprintf(buf, sizeof buf, " grid=%u,%u,%u block=%u lds=%zu\n", g.x, g.y, g.z, b.x, lds);
    g_log += n + buf;
    return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipGetDevice(int*) { return hipErrorNoDevice; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) { g_log += "memcpy\n"; return hipSuccess; }
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int* n, const void*, int, size_t) { *n = 1; return hipSuccess; }
void rec_reset(void) { g_log.clear(); }
const char* rec_log(void) { return g_log.c_str(); }
}
